"""Float64 reference of the sparse compositing operators of csrc/query.hip (test helper, no test functions, no GPU call).

Semantics (include/splat_hip.h, "point tracking"): out [Q, C] = grid_sample(alpha_blending(...), align_corners = True, bilinear,
zero padding) at Q sub-pixel points without the dense image, and the gradient of that expression w.r.t. uv, conic, opacity and
feature.  Written in numpy on top of composite_ref: everything takes a composite_ref.Walk, nothing is imported from the library.

Corners.  The float32 points are taken as exact.  (x0, y0) = floor, the corners nw, ne, sw, se = (x0, y0), (x0 + 1, y0),
(x0, y0 + 1), (x0 + 1, y0 + 1); weights (x1 - ix)(y1 - iy), ... in float64; a corner outside [0, W-1] x [0, H-1] contributes
nothing, a point that is not finite or lies beyond 1e6 has no corner at all.  The LIVE entries (forward_live, the batch forward,
every backward) do not walk an in-image corner whose weight is zero either: its corner maps read 0.

Forward.  out[q, c] = sum_k w_k img64[c, y_k, x_k] with (img64, comp) = composite_ref.forward.  corner_T / corner_ncontrib are the
walk's final_T / ncontrib at the corner pixels, 0 where the corner is not walked.
  Bar of out: K_image sum_k w_k comp[c, y_k, x_k] + COMBINE eps sum_k w_k |img64[c, y_k, x_k]|.  The first term is the dense image's
  bar carried through the bilinear sum.  The second covers what points_corner and the corner combine add, counted per corner term
  s_val[k] * cw[k] (relative errors in units of eps = 2^-24):
      x1 - ix  or  ix - x0        1   (exact for most points; (x0 + 1) - ix rounds where ix is small against 1)
      y1 - iy  or  iy - y0        1
      their product cw            1
      the product s_val * cw      1   (0 where the compiler fuses it into the sum)
      acc += ... , four terms     3   (three additions, each at most eps x the sum of the magnitudes so far)
  = 7 eps x sum_k w_k |value_k|; F + T bg, the rounding that forms s_val, is the dense image's own last step and lies in comp.
  COMBINE = 8 rounds that up.  For a point on eighths the first three lines are exact: the term then only covers the sum.
  Bar of corner_T: K_final_T x Walk.final_T_companion() at the corner pixel; corner_ncontrib is exact.

Backward.  The pixel gradient image G[c, y, x] = sum over the (q, k) on that pixel of w_k(q) g[q, c], in float64; the gradients are
composite_ref.backward(wk, ..., G).  The companions depend on magnitudes only and are taken from A = sum w_k |g[q, c]| (two
queries of opposite sign on one pixel do not shrink the bar); the "n eps x magnitude" term counts corner terms, not pixels
(composite_ref.backward(mult=)), and the geometry gradients count every corner term once per 256-channel launch (geom_mult=).
A detached opacity has no opacity gradient; the others are unchanged.

Batch (the clips of frames_composite_ref).  Every frame carries its own walk and the queries come in CSR form (split()): a frame's
rows are compared with forward / backward of that frame's queries on that frame's walk.  A feature shared by the frames (stride
0) collects the sum of the frames' feature gradients under the sum of their bars; the geometry gradients are compared per frame
after the pair records are reduced per Gaussian, as dense + sparse under the sum of the two bars, because the tile backward of the
same forward wrote the records first (tests/test_gpu_points_reference.py run_batch).

f32_points: the kernels' arithmetic in numpy float32, term by term from the device functions of csrc/query.hip.  It exists to
decide K (tests/test_points_ref_cpu.py) and is not fitted to any GPU output."""
from __future__ import annotations

import dataclasses
import json
import os

import numpy as np

import composite_ref as cr

F32 = np.float32
EPS = cr.EPS
TILE = cr.TILE
COMBINE = 8.0               # see the docstring: 7 roundings per corner term, rounded up
PT_CHUNK = 256              # channels per launch of the sparse kernels (64 lanes x 4 accumulators)
FAR = 1.0e6
KX, KY = np.array([0, 1, 0, 1]), np.array([0, 0, 1, 1])      # nw, ne, sw, se
GRADS = ("uv", "conic", "opacity", "feature")

COMPOSITE_PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "composite_reference_cpu_float32.json")
PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "points_reference_cpu_float32.json")
# sparse output -> the dense output whose K it may reuse
REUSES = dict(out="image", corner_T="final_T", uv="uv", conic="conic", opacity="opacity", feature="feature")


def k_bar():
    """K per sparse output: the dense K of profiles/composite_reference_cpu_float32.json where the reuse condition holds, else the
    sparse K that profiles/points_reference_cpu_float32.json records"""
    dense = json.load(open(COMPOSITE_PROFILE))["K"]
    own = json.load(open(PROFILE)).get("K_own", {}) if os.path.exists(PROFILE) else {}
    return {k: float(own.get(k, dense[d])) for k, d in REUSES.items()}


def dense_k():
    return json.load(open(COMPOSITE_PROFILE))["K"]


# ------------------------------------------------------------------ corners
@dataclasses.dataclass
class Corners:
    px: np.ndarray        # [Q, 4] int, 0 where the corner is outside
    py: np.ndarray
    w: np.ndarray         # [Q, 4] float64 bilinear weights, 0 where the corner is outside
    inside: np.ndarray    # [Q, 4] bool
    live: np.ndarray      # [Q, 4] bool: inside and of non-zero weight
    w32: np.ndarray       # [Q, 4] float32: the weights as points_corner forms them (f32_points only)

    def walked(self, live):
        return self.live if live else self.inside


def corners(points, W, H) -> Corners:
    pts = np.asarray(points, F32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        p = pts.astype(np.float64)
        ok = np.isfinite(p).all(1) & (np.abs(p) <= FAR).all(1)
        ps = np.where(ok[:, None], p, 0.0)
        x0, y0 = np.floor(ps[:, 0]), np.floor(ps[:, 1])
        cx, cy = x0[:, None] + KX[None, :], y0[:, None] + KY[None, :]
        inside = ok[:, None] & (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
        fx, fy = (ps[:, 0] - x0)[:, None], (ps[:, 1] - y0)[:, None]
        w = np.where(KX[None, :] == 1, fx, 1.0 - fx) * np.where(KY[None, :] == 1, fy, 1.0 - fy)
        w = np.where(inside, w, 0.0)
        # points_corner in float32: (k & 1) ? pt.x - x0f : (x0f + 1.f) - pt.x, the same in y, one product
        x0f, y0f = np.floor(pts[:, 0]).astype(F32)[:, None], np.floor(pts[:, 1]).astype(F32)[:, None]
        ptx, pty = pts[:, 0:1], pts[:, 1:2]
        wx32 = np.where(KX[None, :] == 1, ptx - x0f, (x0f + F32(1)) - ptx).astype(F32)
        wy32 = np.where(KY[None, :] == 1, pty - y0f, (y0f + F32(1)) - pty).astype(F32)
        w32 = np.where(inside, (wx32 * wy32).astype(F32), F32(0)).astype(F32)
    px = np.where(inside, cx, 0).astype(np.int64)
    py = np.where(inside, cy, 0).astype(np.int64)
    return Corners(px, py, w, inside, inside & (w != 0), w32)


# ------------------------------------------------------------------ forward
def forward(wk: cr.Walk, feature, bg, points, live=False, co: Corners = None, image=None):
    """dict(out [Q,C], out_comp, out_mag, corner_T [Q,4], corner_T_comp, corner_n [Q,4] int32); image: (img64, comp) of
    composite_ref.forward(wk, feature, bg) where the caller has it already; co: other corners than corners(points) (the fault
    injections of the CPU tests)"""
    img, comp = cr.forward(wk, feature, bg) if image is None else image
    co = corners(points, wk.W, wk.H) if co is None else co
    fT, nc, _ = wk.image_maps()
    cT = wk.final_T_companion()
    v = img[:, co.py, co.px]                      # [C, Q, 4]
    out = (co.w[None] * v).sum(-1).T
    out_comp = (co.w[None] * comp[:, co.py, co.px]).sum(-1).T
    out_mag = (co.w[None] * np.abs(v)).sum(-1).T
    walked = co.walked(live)
    return dict(out=out, out_comp=out_comp, out_mag=out_mag, corner_T=np.where(walked, fT[co.py, co.px], 0.0),
                corner_T_comp=np.where(walked, cT[co.py, co.px], 0.0), corner_n=np.where(walked, nc[co.py, co.px], 0).astype(np.int32))


def out_companion(ref, K_image):
    """the companion of out: K_image x it is the bar of the docstring"""
    return ref["out_comp"] + COMBINE * EPS * ref["out_mag"] / K_image


# ------------------------------------------------------------------ backward
def pixel_gradient(co: Corners, g, W, H):
    """(G [C,H,W] = sum w_k g, A = sum w_k |g|, M [H,W] = corner terms per pixel) over the live corners"""
    g = np.asarray(g, np.float64)
    C = g.shape[1]
    G, A, M = np.zeros((C, H, W)), np.zeros((C, H, W)), np.zeros((H, W))
    for k in range(4):
        m = co.live[:, k]
        idx = (slice(None), co.py[m, k], co.px[m, k])
        np.add.at(G, idx, (co.w[m, k, None] * g[m]).T)
        np.add.at(A, idx, (co.w[m, k, None] * np.abs(g[m])).T)
        np.add.at(M, (co.py[m, k], co.px[m, k]), 1.0)
    return G, A, M


def backward(wk: cr.Walk, conic, opacity, feature, bg, points, g, detach_opacity=False, co: Corners = None, companions=True):
    """(grads, comps): dicts over uv [N,2], conic [N,3], opacity [N] (absent when detached), feature [N,C]"""
    co = corners(points, wk.W, wk.H) if co is None else co
    C = np.asarray(feature).shape[1]
    G, A, M = pixel_gradient(co, g, wk.W, wk.H)
    grads, comps = cr.backward(wk, conic, opacity, feature, bg, G, companions=companions, dL_mag=A, mult=M,
                               geom_mult=(C + PT_CHUNK - 1) // PT_CHUNK)
    keep = [k for k in GRADS if not (detach_opacity and k == "opacity")]
    return {k: grads[k] for k in keep}, (None if comps is None else {k: comps[k] for k in keep})


# ------------------------------------------------------------------ frame batch (clips of frames_composite_ref)
def split(offsets, a):
    """the rows of frame f of a CSR array"""
    o = np.asarray(offsets).astype(np.int64)
    return [np.asarray(a)[o[f]:o[f + 1]] for f in range(o.size - 1)]


# ------------------------------------------------------------------ float32 restatement of csrc/query.hip
def _f(x):
    return np.asarray(x, F32)


def f32_points(uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, points, dL_dout=None, live=True,
               detach_opacity=False):
    """The sparse kernels' arithmetic in numpy float32:
      points_corner     floor, the two differences and their product in float32
      points_entry      composite_ref.f32_tile_alpha: power_coeffs / power_poly / exp2 / clamps about the corner's tile centre
      the chain         over the entries that passed alpha >= 1/255, in list order: nT = T (1 - a); nT < 1e-4 ends the corner
                        unapplied; an applied entry leaves its weight a T
      channels          F[c] = fma(f[id, c], weight, F[c]) in list order
      corner combine    s_val = fma(T, bg, F); acc = fma(s_val[k], cw[k], acc) over the corners inside the image, nw ne sw se
      backward          per live corner (cw != 0, corner_ncontrib > 0) and launch of 256 channels: g = cw dL_dout, bgdot = bg sum g;
                        back to front from corner_T: T = T rcp(1 - a), weight = a T, dLa = (sum_c (f_c - acc_c) g_c) T
                        + (-Tf rcp(1 - a)) bgdot, dL_dfeature += weight g, acc = a f + (1 - a) acc
      points_geo_terms  the direct form dx = u - px: G = araw rcp(o), dLG = o dLa; uv: dLG (-G dx cA - G dy cB), ...; conic:
                        (-0.5 G dx dx) dLG, ...; opacity: G dLa; every launch ADDS its terms (one rounding per add)
    Returns dict(out, corner_T, corner_n, grads or None)."""
    uv, conic = _f(uv).reshape(-1, 2), _f(conic).reshape(-1, 3)
    op = _f(opacity).reshape(-1)
    f = _f(feature)
    N, C = f.shape
    idx = np.asarray(idx_sorted).reshape(-1).astype(np.int64)
    tr = np.asarray(tile_range).reshape(-1, 2).astype(np.int64)
    pts = _f(points).reshape(-1, 2)
    Q = pts.shape[0]
    co = corners(pts, W, H)
    gx = (W + TILE - 1) // TILE
    bgf = F32(bg)
    one, tmin = F32(1), F32(0.0001)
    tiles, pixels = {}, {}

    def tile_of(tx, ty):
        if (tx, ty) not in tiles:
            t = ty * gx + tx
            ids = idx[int(tr[t, 0]):int(tr[t, 1])]
            x0, y0 = tx * TILE, ty * TILE
            nx, ny = min(W, x0 + TILE) - x0, min(H, y0 + TILE) - y0
            with np.errstate(all="ignore"):
                alpha, raw, _, _ = cr.f32_tile_alpha(uv, conic, op, ids, x0, y0, nx, ny)
            tiles[(tx, ty)] = (ids, alpha, raw, x0, y0, nx)
        return tiles[(tx, ty)]

    def pixel(px, py):
        """the forward walk of one corner pixel: (ids, applied positions, their alphas and raw alphas, T, last, F + T bg)"""
        if (px, py) not in pixels:
            ids, alpha, raw, x0, y0, nx = tile_of(px // TILE, py // TILE)
            p = (py - y0) * nx + (px - x0)
            a = alpha[:, p] if ids.size else np.zeros(0, F32)
            T, last, app, wts = one, 0, [], []
            for i in np.nonzero(a != 0)[0]:
                nT = F32(T * F32(one - a[i]))
                if nT < tmin:
                    break
                wts.append(F32(a[i] * T))
                app.append(int(i))
                T, last = nT, int(i) + 1
            Facc = np.zeros(C, F32)
            for i, wg in zip(app, wts):
                Facc = cr._fma(f[ids[i]], wg, Facc)
            val = cr._fma(T, bgf, Facc)
            app = np.asarray(app, np.int64)
            pixels[(px, py)] = (ids, app, a[app] if app.size else np.zeros(0, F32), raw[app, p] if app.size else np.zeros(0, F32), T, last, val)
        return pixels[(px, py)]

    out = np.zeros((Q, C), F32)
    cT, cn = np.zeros((Q, 4), F32), np.zeros((Q, 4), np.int32)
    walked = co.walked(live)
    with np.errstate(all="ignore"):
        for q in range(Q):
            acc = np.zeros(C, F32)
            for k in range(4):
                if not co.inside[q, k]:
                    continue
                if walked[q, k]:
                    _, _, _, _, T, last, val = pixel(int(co.px[q, k]), int(co.py[q, k]))
                    cT[q, k], cn[q, k] = T, last
                else:       # a weightless corner of a LIVE walk: F = 0, T = 1, so s_val = bg, times cw = 0
                    val = np.full(C, bgf, F32)
                acc = cr._fma(val, co.w32[q, k], acc)
            out[q] = acc
    grads = None
    if dL_dout is not None:
        dL = _f(dL_dout).reshape(Q, C)
        grads = dict(uv=np.zeros((N, 2), F32), conic=np.zeros((N, 3), F32), opacity=np.zeros(N, F32), feature=np.zeros((N, C), F32))
        half = F32(-0.5)
        with np.errstate(all="ignore"):
            for c0 in range(0, C, PT_CHUNK):        # launches on one stream: chunks ascending
                c1 = min(C, c0 + PT_CHUNK)
                for q in range(Q):
                    for k in range(4):
                        cw = co.w32[q, k]
                        if not co.inside[q, k] or cw == 0 or cn[q, k] <= 0:
                            continue
                        px, py = int(co.px[q, k]), int(co.py[q, k])
                        ids, app, al, araw, Tf, last, _ = pixel(px, py)
                        pxf, pyf = F32(px), F32(py)
                        g = (cw * dL[q, c0:c1]).astype(F32)
                        bgdot = F32(bgf * g.sum(dtype=F32))
                        T = Tf
                        acc = np.zeros(c1 - c0, F32)
                        for j in range(app.size - 1, -1, -1):
                            i = int(ids[app[j]])
                            a = al[j]
                            om = F32(one - a)
                            r1a = F32(one / om)
                            T = F32(T * r1a)
                            wgt = F32(a * T)
                            fr = f[i, c0:c1]
                            part = (((fr - acc).astype(F32)) * g).astype(F32).sum(dtype=F32)
                            dLa = F32(part * T)
                            dLa = F32(dLa + F32(F32(-Tf * r1a) * bgdot))
                            grads["feature"][i, c0:c1] += (wgt * g).astype(F32)
                            acc = ((a * fr).astype(F32) + (om * acc).astype(F32)).astype(F32)
                            # points_geo_terms
                            u_, v_, cA, cB, cC, o = uv[i, 0], uv[i, 1], conic[i, 0], conic[i, 1], conic[i, 2], op[i]
                            dx, dy = F32(u_ - pxf), F32(v_ - pyf)
                            G = F32(araw[j] * F32(one / o))
                            dLG = F32(o * dLa)
                            bux = F32(F32(F32(-G * dx) * cA) - F32(F32(G * dy) * cB))
                            buy = F32(F32(F32(-G * dy) * cC) - F32(F32(G * dx) * cB))
                            grads["uv"][i, 0] += F32(dLG * bux)
                            grads["uv"][i, 1] += F32(dLG * buy)
                            grads["conic"][i, 0] += F32(F32(F32(F32(half * G) * dx) * dx) * dLG)
                            grads["conic"][i, 1] += F32(F32(F32(-G * dx) * dy) * dLG)
                            grads["conic"][i, 2] += F32(F32(F32(F32(half * G) * dy) * dy) * dLG)
                            if not detach_opacity:
                                grads["opacity"][i] += F32(G * dLa)
        if detach_opacity:
            del grads["opacity"]
    return dict(out=out, corner_T=cT, corner_n=cn, grads=grads)


# ------------------------------------------------------------------ query sets of the tests
def queries(W, H, seed=0, crowd_tile=None, nonfinite=True):
    """[Q, 2] float32 and names -> index arrays.  Most points lie on eighths of a pixel (exact float32 weights); the groups:
      eighths     seeded, uniform over [-1, W] x [-1, H] (a rim outside the image included), rounded to eighths
      free        seeded float32 points that are on no grid
      integer     integer pixels (one live corner each), the image's corners among them
      straddle    points whose four corners lie in four tiles
      edge        corners in the last column and the last row (partial tiles) and in the top right tile
      half        half outside: two corners (or one) in the image
      outside     no corner in the image (a far point among them)
      repeat      copies of earlier queries; pairs of different queries that share a corner pixel
      crowd       20 points inside the tile ``crowd_tile`` = (tx, ty): 80 live corners for one wave of the ordered route
      nonfinite   NaN and inf coordinates (nonfinite = True)"""
    rng = np.random.default_rng(500 + seed)
    groups, rows = {}, []

    def add(name, a):
        a = np.asarray(a, np.float64).reshape(-1, 2)
        groups[name] = np.arange(len(rows), len(rows) + len(a))
        rows.extend(a.tolist())

    add("eighths", np.round(rng.uniform([-1, -1], [W, H], size=(96, 2)) * 8) / 8)
    add("free", rng.uniform([0, 0], [W - 1, H - 1], size=(24, 2)).astype(F32))
    gxn, gyn = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    ints = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)] + [(int(x), int(y)) for x, y in rng.integers([1, 1], [W - 1, H - 1], size=(28, 2))]
    add("integer", ints)
    strad = [(16 * i - 0.5 + dx, 16 * j - 0.5 + dy) for i in range(1, gxn) for j in range(1, gyn) if 16 * i < W and 16 * j < H
             for dx, dy in ((0.0, 0.0), (0.25, -0.125))]
    add("straddle", strad)
    add("edge", [(W - 1.5, 20.25), (W - 2.25, H - 1.5), (W - 1.125, 3.5), (W - 3.5, 9.75), (W - 2.5, 1.25), (10.5, H - 1.25),
                 (40.375, H - 2.5), (W - 1.75, H - 1.75), (W - 1.0, 7.5), (33.5, H - 1.0)])
    add("half", [(-0.5, 10.5), (W - 0.5, 20.25), (30.5, H - 0.75), (-0.25, -0.25), (W - 0.625, H - 0.5), (12.25, -0.875)])
    add("outside", [(-3.0, 5.0), (W + 2.0, 5.0), (1.0e9, 3.0), (5.5, -1.0), (-1.0, -1.0), (7.0, H + 0.0)])
    if crowd_tile is not None:
        tx, ty = crowd_tile
        add("crowd", np.round(rng.uniform([16 * tx + 0.5, 16 * ty + 0.5], [16 * tx + 14.5, 16 * ty + 14.5], size=(20, 2)) * 8) / 8)
    e = groups["eighths"]
    rep = [rows[e[0]], rows[e[0]], rows[e[5]], rows[groups["integer"][5]], rows[groups["straddle"][0]]]
    rep += [(20.25, 10.5), (20.75, 10.25), (20.5, 10.5), (50.125, 40.5), (50.875, 40.75)]
    add("repeat", rep)
    if nonfinite:
        add("nonfinite", [(np.nan, 3.0), (4.0, np.inf), (-np.inf, np.nan)])
    return np.asarray(rows, np.float64).astype(F32), groups


def one_query_per_tile(co: Corners, W):
    """[Q] bool: for every tile the first query whose nw corner is live in it"""
    gx = (W + TILE - 1) // TILE
    pick, seen = np.zeros(co.px.shape[0], bool), set()
    for q in range(co.px.shape[0]):
        if co.live[q, 0]:
            t = (int(co.py[q, 0]) // TILE) * gx + int(co.px[q, 0]) // TILE
            if t not in seen:
                seen.add(t)
                pick[q] = True
    return pick


def coverage(wk: cr.Walk, tr, points):
    """facts about a query set on a walk that the tests assert"""
    co = corners(points, wk.W, wk.H)
    gx, gy = (wk.W + TILE - 1) // TILE, (wk.H + TILE - 1) // TILE
    fT, nc, _ = wk.image_maps()
    n = (np.asarray(tr).reshape(-1, 2)[:, 1] - np.asarray(tr).reshape(-1, 2)[:, 0]).astype(int)
    stopped = np.zeros((wk.H, wk.W), bool)
    for t in wk.tiles:
        stopped[t.y0:t.y0 + t.ny, t.x0:t.x0 + t.nx] = t.stopped.reshape(t.ny, t.nx)
    tile = (co.py // TILE) * gx + co.px // TILE
    lv = co.live
    p64 = np.nan_to_num(np.asarray(points, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    per_tile = np.bincount(tile[lv & (nc[co.py, co.px] > 0)], minlength=gx * gy)
    four = int(sum(1 for q in range(tile.shape[0]) if lv[q].all() and np.unique(tile[q]).size == 4))
    hits = np.zeros((wk.H, wk.W), int)
    np.add.at(hits, (co.py[lv], co.px[lv]), 1)
    qhits = np.zeros((wk.H, wk.W), int)                 # different queries per pixel
    for q in range(tile.shape[0]):
        m = lv[q]
        qhits[co.py[q, m], co.px[q, m]] += 1
    return dict(live=int(lv.sum()), live_in_tile=lambda tx, ty: int((lv & (tile == ty * gx + tx)).sum()),
                in_empty_tiles=int((co.inside & (n[tile] == 0)).sum()),
                last_column=int((lv & (co.px // TILE == gx - 1)).sum()), last_row=int((lv & (co.py // TILE == gy - 1)).sum()),
                past_first_block=int((lv & (nc[co.py, co.px] >= 65)).sum()), stopped=int((lv & stopped[co.py, co.px]).sum()),
                four_tiles=four, shared_pixels=int((qhits >= 2).sum()), most_live_in_a_tile=int(per_tile.max()),
                weightless=int((co.inside & ~lv).sum()), half_outside=int(((co.inside.sum(1) > 0) & (co.inside.sum(1) < 4)).sum()),
                outside=int((co.inside.sum(1) == 0).sum()),
                off_eighths=int((np.abs(p64 * 8 - np.round(p64 * 8)) > 0).any(1).sum()),
                lists_of=lambda ids: int(sum(1 for q in range(tile.shape[0]) for k in range(4) if lv[q, k] and
                                             np.isin(ids, wk.tiles[tile[q, k]].ids).any())))
