"""Float64 alpha compositing with decision margins and magnitude companions (test helper).

Written in numpy from the operator semantics, vectorised over the pixels of a tile; independent of torch_twin.blend (which
the CPU tests use as a cross-check).  The inputs are the float32 operands the kernels receive, taken as exact.

Rules (csrc/blend_power.h, include/splat_hip.h):
  raw alpha a = min(o exp(power), 1), no separate "power > 0" skip; a non-finite a counts as skipped;
  alpha = min(a (+ bias), 0.99), the clamp straight-through in the gradient; skip when alpha < 1/255;
  stop WITHOUT applying when T (1 - alpha) < 1e-4; with truncation a pixel ends after K recorded contributors;
  ncontrib = list position (1-based) of the last applied entry; gs_idx = the first K applied ids, padded with -1.

Error model, eps = 2^-24, per evaluation (pixel p, entry i):
  M_pi     every term of the tile-centred polynomial q0 + qx x + qy y + qxx x^2 + qxy x y + qyy y^2 of power_coeffs() /
           power_poly() and of its coefficients taken over magnitudes (log2 units, |log2 o| included);
  e_alpha  = eps (ln2 M_pi + 2), the relative error of the raw alpha; with a bias it enters alpha absolutely,
           d_alpha = e_alpha a + eps (a + |bias|);
  E_T(p,i) = sum over the applied entries before i of d_alpha / (1 - alpha) + eps.
Decisions: alpha vs 1/255 is CLEAR when |ln(255 alpha)| >= S d_alpha / alpha; the stop is clear when
|ln(T (1 - alpha) / 1e-4)| >= S (E_T + d_alpha / (1 - alpha)); S = 8 is a condition, not a measurement.  (The bias operator
evaluates the reference's factored form and skips when it comes out negative: clear when -power >= S eps x its magnitudes.)
prune() removes every Gaussian with an unclear decision on a live pixel until none is left: on a pruned scene float32 and
float64 walk the same way, so integer outputs compare exactly and values within K x companion.

Companions: the forward / backward sums once more with every product and sum taken over magnitudes (dx as |u - cx| + |x|:
the kernels obtain the gradients from moments about a centre, so their rounding scales with the expanded terms), each term
weighted by the relative error accumulated at its entry, plus n eps x the magnitude sum for a sum of n terms in any order
(float atomics, every reduction tree)."""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

TILE = 16
EPS = 2.0 ** -24
LN2 = float(np.log(2.0))
L2E = 1.0 / LN2
A_MIN = 1.0 / 255.0
T_MIN = 1e-4
A_MAX = 0.99
S_CLEAR = 8.0
TINY = 2.0 ** -126   # smallest normal float32: what a flushed denormal loses
CHUNK = 32          # channels per backward pass: |d uv| is summed per chunk


@dataclasses.dataclass
class TileWalk:
    tile: int
    x0: int
    y0: int
    nx: int
    ny: int
    ids: np.ndarray        # [n] Gaussian ids of the walked entries (the list up to where every pixel had ended)
    nlist: int             # length of the tile's list
    alpha: np.ndarray      # [n, P]
    araw: np.ndarray       # [n, P] o exp(power) (d alpha / d power)
    G: np.ndarray          # [n, P] exp(power)
    applied: np.ndarray    # [n, P] bool
    Tb: np.ndarray         # [n, P] transmittance in front of the entry
    ET: np.ndarray         # [n, P] E_T in front of the entry
    ea: np.ndarray         # [n, P] relative error of alpha (d_alpha / alpha), 0 where not applied
    er: np.ndarray         # [n, P] relative error of o exp(power) and of exp(power) (e_alpha of the raw term), 0 where not applied
    dx: np.ndarray         # [n, P] u - px
    dy: np.ndarray
    mdx: np.ndarray        # [n, P] |u - cx| + |x|
    mdy: np.ndarray
    Tf: np.ndarray         # [P]
    ETf: np.ndarray        # [P]
    last: np.ndarray       # [P] int
    stopped: np.ndarray    # [P] bool: the pixel ended before its list did (saturation or truncation)
    gs: np.ndarray         # [P, max(K, 1)] int
    unclear: np.ndarray    # [n] bool: some live pixel has an unclear decision on this entry
    Mmax: float

    @property
    def w(self):
        return np.where(self.applied, self.alpha * self.Tb, 0.0)


@dataclasses.dataclass
class Walk:
    W: int
    H: int
    N: int
    K: int
    tiles: list
    has_bias: bool

    def unclear_ids(self):
        out = [t.ids[t.unclear] for t in self.tiles]
        return np.unique(np.concatenate(out)) if out else np.zeros(0, np.int64)

    def evaluations(self):
        return int(sum(t.alpha.size for t in self.tiles))

    def Mmax(self):
        return max([t.Mmax for t in self.tiles] + [0.0])

    def image_maps(self):
        """final_T [H,W], ncontrib [H,W] int32, gs_idx [H,W,K]"""
        fT = np.ones((self.H, self.W))
        nc = np.zeros((self.H, self.W), np.int32)
        gi = np.full((self.H, self.W, max(self.K, 1)), -1, np.int32)
        for t in self.tiles:
            sl = (slice(t.y0, t.y0 + t.ny), slice(t.x0, t.x0 + t.nx))
            fT[sl] = t.Tf.reshape(t.ny, t.nx)
            nc[sl] = t.last.reshape(t.ny, t.nx)
            gi[sl] = t.gs.reshape(t.ny, t.nx, -1)
        return fT, nc, gi

    def final_T_companion(self):
        c = np.zeros((self.H, self.W))
        for t in self.tiles:
            c[t.y0:t.y0 + t.ny, t.x0:t.x0 + t.nx] = (t.Tf * (t.ETf + EPS)).reshape(t.ny, t.nx)
        return c


def _f64(a):
    return np.asarray(a, np.float64)


def walk(uv, conic, opacity, idx_sorted, tile_range, W, H, bias=None, K=0, truncate=False) -> Walk:
    uv, conic = _f64(uv).reshape(-1, 2), _f64(conic).reshape(-1, 3)
    op = _f64(opacity).reshape(-1)
    bs = None if bias is None else _f64(bias).reshape(-1)
    idx = np.asarray(idx_sorted).reshape(-1).astype(np.int64)
    tr = np.asarray(tile_range).reshape(-1, 2).astype(np.int64)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tiles = []
    with np.errstate(all="ignore"):
        for tile in range(gx * gy):
            tiles.append(_walk_tile(tile, gx, uv, conic, op, bs, idx, tr, W, H, K, truncate))
    return Walk(W, H, uv.shape[0], K, tiles, bias is not None)


def poly_magnitude(uc, vc, aA, aB, aC, o, x, y):
    """M: the terms of power_coeffs() and power_poly() over magnitudes, log2 units; uc, vc = |centre - tile centre|, x, y =
    |pixel - tile centre|, aA .. aC = |conic|"""
    mtx, mty = aA * uc + aB * vc, aB * uc + aC * vc
    return np.abs(np.log2(o)) + L2E * (0.5 * (uc * mtx + vc * mty) + mtx * x + mty * y + 0.5 * aA * x * x + aB * x * y + 0.5 * aC * y * y)


def alpha_decisions_clear(u, v, cA, cB, cC, o, W, H):
    """whether one splat's alpha >= 1/255 decision is clear on EVERY pixel of the image (each pixel with its tile's centre)"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cx, cy = np.floor(xs / TILE) * TILE + 7.5, np.floor(ys / TILE) * TILE + 7.5
    u, v, cA, cB, cC, o = (float(a) for a in (u, v, cA, cB, cC, o))
    dx, dy = u - xs, v - ys
    with np.errstate(all="ignore"):
        a = np.minimum(o * np.exp(-0.5 * (cA * dx * dx + cC * dy * dy) - cB * dx * dy), 1.0)
        M = poly_magnitude(np.abs(u - cx), np.abs(v - cy), abs(cA), abs(cB), abs(cC), o, np.abs(xs - cx), np.abs(ys - cy))
        e = EPS * (LN2 * M + 2.0)
        return bool((np.abs(np.log(np.where(a > 0, a, 1.0) * 255.0)) >= S_CLEAR * e)[a > 0].all())


def _walk_tile(tile, gx, uv, conic, op, bs, idx, tr, W, H, K, truncate) -> TileWalk:
    tx, ty = tile % gx, tile // gx
    x0, y0 = tx * TILE, ty * TILE
    nx, ny = min(W, x0 + TILE) - x0, min(H, y0 + TILE) - y0
    ys, xs = np.meshgrid(np.arange(y0, y0 + ny), np.arange(x0, x0 + nx), indexing="ij")
    px, py = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64)
    P = px.size
    cx, cy = x0 + 7.5, y0 + 7.5
    r0, r1 = int(tr[tile, 0]), int(tr[tile, 1])
    ids = idx[r0:r1]
    n = ids.size
    u, v = uv[ids, 0][:, None], uv[ids, 1][:, None]
    cA, cB, cC = (conic[ids, k][:, None] for k in range(3))
    o = op[ids][:, None]
    dx, dy = u - px[None, :], v - py[None, :]
    power = -0.5 * (cA * dx * dx + cC * dy * dy) - cB * dx * dy
    G = np.exp(power)
    oG = o * G
    araw = np.minimum(oG, 1.0)
    # ---- magnitudes of the tile-centred polynomial (log2 units)
    x, y = np.abs(px - cx)[None, :], np.abs(py - cy)[None, :]
    uc, vc = np.abs(u - cx), np.abs(v - cy)
    aA, aB, aC = np.abs(cA), np.abs(cB), np.abs(cC)
    M = poly_magnitude(uc, vc, aA, aB, aC, o, x, y)
    e_raw = EPS * (LN2 * M + 2.0)
    if bs is None:
        a_in = araw
        d_alpha = e_raw * araw
        sign_ok = np.ones_like(araw, bool)
        sign_clear = sign_ok
    else:
        b = bs[ids][:, None]
        a_in = oG + b                 # the bias operator: fma(o, exp(power), bias), no clamp of the raw term
        d_alpha = e_raw * oG + EPS * (oG + np.abs(b))
        mq = 0.5 * aA * dx * dx + aB * np.abs(dx * dy) + 0.5 * aC * dy * dy
        sign_ok = ~(-power < 0)       # skipped when the factored form is negative
        sign_clear = (-power >= S_CLEAR * 4.0 * EPS * mq) | ((dx == 0) & (dy == 0))
        araw = oG
    alpha = np.minimum(a_in, A_MAX)
    finite = np.isfinite(a_in) & np.isfinite(power)
    valid = finite & sign_ok & (alpha >= A_MIN)
    # alpha decision: non-finite operands and alpha = 0 are skipped whatever the rounding
    pos = finite & (alpha > 0)
    rel = np.where(pos, d_alpha / np.where(pos, alpha, 1.0), 0.0)
    lnm = np.abs(np.log(np.where(pos, alpha, 1.0) * 255.0))
    clear_a = np.where(pos, lnm >= S_CLEAR * rel, True)
    neg = finite & (alpha <= 0) & (alpha != 0)
    clear_a = np.where(neg, (A_MIN - alpha) >= S_CLEAR * d_alpha, clear_a)
    clear_a &= np.where(finite, sign_clear | (alpha < A_MIN), True)
    clear_a = np.where(finite & ~np.isfinite(M) & (alpha > 0), False, clear_a)
    one_m = 1.0 - alpha
    dT = np.where(valid, d_alpha / np.where(valid, one_m, 1.0), 0.0)

    T = np.ones(P)
    ET = np.zeros(P)
    done = np.zeros(P, bool)
    last = np.zeros(P, np.int64)
    layer = np.zeros(P, np.int64)
    gs = np.full((P, max(K, 1)), -1, np.int64)
    Tb, ETb = np.ones((n, P)), np.zeros((n, P))
    applied = np.zeros((n, P), bool)
    unclear = np.zeros(n, bool)
    nw = n
    for i in range(n):
        if done.all():
            nw = i
            break
        live = ~done
        ok = live & valid[i]
        nT = T * one_m[i]
        sat = ok & (nT < T_MIN)
        app = ok & ~sat
        stop_clear = np.abs(np.log(np.where(ok, nT, 1.0) / T_MIN)) >= S_CLEAR * (ET + dT[i])
        unclear[i] = bool((live & ~clear_a[i]).any() or (ok & ~stop_clear).any())
        Tb[i], ETb[i], applied[i] = T, ET, app
        T = np.where(app, nT, T)
        ET = ET + np.where(app, dT[i] + EPS, 0.0)
        last = np.where(app, i + 1, last)
        done |= sat
        if K > 0:
            rec = app & (layer < K)
            if rec.any():
                r = np.nonzero(rec)[0]
                gs[r, layer[r]] = ids[i]
                layer = layer + rec
            if truncate:
                done |= app & (layer >= K)
    s = slice(0, nw)
    z = lambda a: np.where(applied[s], a[s], 0.0)
    mdx = np.broadcast_to(uc, (n, P)) + x
    mdy = np.broadcast_to(vc, (n, P)) + y
    Mw = np.where(applied[s], M[s], 0.0)
    return TileWalk(tile, x0, y0, nx, ny, ids[s], n, z(alpha), z(araw), z(G), applied[s], Tb[s], ETb[s], z(rel), z(e_raw), z(dx), z(dy),
                    z(mdx), z(mdy), T, ET, last, done.copy(), gs, unclear[s], float(Mw.max()) if Mw.size else 0.0)


# ------------------------------------------------------------------ forward
def _bg_vec(bg, C):
    b = np.asarray(bg, np.float64).reshape(-1)
    return np.full(C, float(b[0])) if b.size == 1 else b


def forward(wk: Walk, feature, bg):
    """image [C,H,W] and its companion (bar = K_image x companion)"""
    f = _f64(feature)
    C = f.shape[1]
    bgv = _bg_vec(bg, C)
    img, comp = np.zeros((C, wk.H, wk.W)), np.zeros((C, wk.H, wk.W))
    for t in wk.tiles:
        w = t.w
        ft, fa = f[t.ids], np.abs(f[t.ids])
        val = w.T @ ft + t.Tf[:, None] * bgv[None, :]
        mag = w.T @ fa + t.Tf[:, None] * np.abs(bgv)[None, :]
        err = (w * (t.ET + t.ea + EPS)).T @ fa + (t.Tf * (t.ETf + EPS))[:, None] * np.abs(bgv)[None, :]
        napp = t.applied.sum(0)
        cmp_ = err + EPS * (napp[:, None] + 1) * mag
        sl = (slice(None), slice(t.y0, t.y0 + t.ny), slice(t.x0, t.x0 + t.nx))
        img[sl] = val.T.reshape(C, t.ny, t.nx)
        comp[sl] = cmp_.T.reshape(C, t.ny, t.nx)
    return img, comp


# ------------------------------------------------------------------ analytic backward
GRADS = ("uv", "conic", "opacity", "feature", "bias", "abs_uv")


def backward(wk: Walk, conic, opacity, feature, bg, dL_dout, companions=True, dL_mag=None, mult=None, geom_mult=1):
    """The back-to-front recurrence, written out:  dL/dalpha_i = T_i f_i.g - S_after_i / (1 - alpha_i),
    S_after_i = sum_{j > i} w_j f_j.g + T_final bg.g;  dL/dpower = dL/dalpha o exp(power) (straight-through clamp).
    Returns (grads, comps): dicts over GRADS; abs_uv sums |.| of the uv terms per chunk of 32 channels.
    For a pixel gradient that is itself a sum of several terms (tests/points_ref.py: the corner terms of sparse queries):
    dL_mag [C,H,W] = the sum of the terms' magnitudes, which the companions then use instead of |dL_dout|; mult [H,W] = the
    terms per pixel, counted instead of 1 in the "n eps x magnitude" term; geom_mult = how often every term is added to the
    geometry gradients (once per launch over a chunk of channels).  The defaults leave every result as it was, bit for bit."""
    f = _f64(feature)
    N, C = f.shape
    cn = _f64(conic).reshape(-1, 3)
    gim = _f64(dL_dout).reshape(C, wk.H, wk.W)
    gmag = None if dL_mag is None else _f64(dL_mag).reshape(C, wk.H, wk.W)
    pmult = None if mult is None else _f64(mult).reshape(wk.H, wk.W)
    bgv = _bg_vec(bg, C)
    shp = dict(uv=(N, 2), conic=(N, 3), opacity=(N,), feature=(N, C), bias=(N,), abs_uv=(N, 2))
    g = {k: np.zeros(s) for k, s in shp.items()}
    ce = {k: np.zeros(s) for k, s in shp.items()}      # error-weighted magnitude sums
    cm = {k: np.zeros(s) for k, s in shp.items()}      # plain magnitude sums
    cnt = np.zeros(N)                                  # pixel terms per Gaussian
    for t in wk.tiles:
        if t.ids.size == 0:
            continue
        ids = t.ids
        gp_ = gim[:, t.y0:t.y0 + t.ny, t.x0:t.x0 + t.nx].reshape(C, -1)        # [C, P]
        w, app = t.w, t.applied
        one_m = 1.0 - t.alpha
        cA, cB, cC = (cn[ids, k][:, None] for k in range(3))
        cA, cB, cC = (np.where(app, c, 0.0) for c in (cA, cB, cC))             # (non-finite rows apply nowhere)
        ft = f[ids]
        g["feature"][ids] += w @ gp_.T
        dLa = np.zeros_like(w)
        for c0 in range(0, C, CHUNK):
            c1 = min(C, c0 + CHUNK)
            fg = ft[:, c0:c1] @ gp_[c0:c1]                                      # [n, P]
            wf = w * fg
            S_after = np.cumsum(wf[::-1], 0)[::-1] - wf + (t.Tf * (bgv[c0:c1] @ gp_[c0:c1]))[None, :]
            dk = np.where(app, t.Tb * fg - S_after / one_m, 0.0)
            gpw = dk * t.araw
            g["abs_uv"][ids, 0] += np.abs(gpw * (-cA * t.dx - cB * t.dy)).sum(1)
            g["abs_uv"][ids, 1] += np.abs(gpw * (-cC * t.dy - cB * t.dx)).sum(1)
            dLa += dk
        gpw = dLa * t.araw
        g["uv"][ids, 0] += (gpw * (-cA * t.dx - cB * t.dy)).sum(1)
        g["uv"][ids, 1] += (gpw * (-cC * t.dy - cB * t.dx)).sum(1)
        g["conic"][ids, 0] += (-0.5 * gpw * t.dx * t.dx).sum(1)
        g["conic"][ids, 1] += (-gpw * t.dx * t.dy).sum(1)
        g["conic"][ids, 2] += (-0.5 * gpw * t.dy * t.dy).sum(1)
        g["opacity"][ids] += (dLa * t.G).sum(1)
        g["bias"][ids] += dLa.sum(1)
        if not companions:
            continue
        # ---- the same sums over magnitudes, each term weighted by the error accumulated at its entry
        ga, fa = np.abs(gp_), np.abs(ft)
        if gmag is not None:
            ga = gmag[:, t.y0:t.y0 + t.ny, t.x0:t.x0 + t.nx].reshape(C, -1)
        napp = app.sum(0)
        R = t.ETf + (napp + C + 8) * EPS                                       # [P]: transmittance (either direction), sums, dot
        r = np.where(app, R[None, :] + t.ea * (1.0 + t.alpha / one_m), 0.0)
        fga = fa @ ga
        wfa = w * fga
        bga = t.Tf * (np.abs(bgv) @ ga)
        rc = lambda a: np.cumsum(a[::-1], 0)[::-1] - a
        magS = rc(wfa) + bga[None, :]
        errS = rc(wfa * r) + (bga * R)[None, :]
        magL = np.where(app, t.Tb * fga + magS / one_m, 0.0)
        errL = np.where(app, t.Tb * fga * r + (errS + magS * r) / one_m, 0.0)
        mp = magL * t.araw
        # o exp(power) and exp(power) carry the polynomial's relative error and, near the bottom of the float32 range, the
        # absolute one of a flushed denormal
        ep = (errL + magL * 8 * EPS) * t.araw + magL * (t.er * t.araw + np.where(app, TINY, 0.0))
        aA, aB, aC = np.abs(cA), np.abs(cB), np.abs(cC)
        geo = dict(uv0=aA * t.mdx + aB * t.mdy, uv1=aC * t.mdy + aB * t.mdx, c0=0.5 * t.mdx * t.mdx, c1=t.mdx * t.mdy,
                   c2=0.5 * t.mdy * t.mdy)
        for k, (name, col) in dict(uv0=("uv", 0), uv1=("uv", 1), c0=("conic", 0), c1=("conic", 1), c2=("conic", 2)).items():
            ce[name][ids, col] += (ep * geo[k]).sum(1)
            cm[name][ids, col] += (mp * geo[k]).sum(1)
        Gm = t.G
        ce["opacity"][ids] += ((errL + magL * 8 * EPS) * Gm + magL * (t.er * Gm + np.where(app, TINY, 0.0))).sum(1)
        cm["opacity"][ids] += (magL * Gm).sum(1)
        ce["bias"][ids] += errL.sum(1)
        cm["bias"][ids] += magL.sum(1)
        ce["feature"][ids] += (w * (t.ET + t.ea + 2 * EPS)) @ ga.T
        cm["feature"][ids] += w @ ga.T
        if pmult is None:
            cnt[ids] += app.sum(1)
        else:
            cnt[ids] += (app * pmult[t.y0:t.y0 + t.ny, t.x0:t.x0 + t.nx].reshape(1, -1)).sum(1)
    if not companions:
        return g, None
    ce["abs_uv"], cm["abs_uv"] = ce["uv"], cm["uv"]
    comps = {}
    for k in GRADS:
        n = cnt.reshape((N,) + (1,) * (len(shp[k]) - 1))
        if geom_mult != 1 and k not in ("feature",):
            n = n * geom_mult
        comps[k] = ce[k] + (n + 4) * EPS * cm[k]
    return g, comps


# ------------------------------------------------------------------ pruning
def prune(uv, conic, opacity, depth, radius, tiles, W, H, sort, bias=None, K=0, truncate=False, max_passes=12):
    """sort(radius) -> (idx_sorted, tile_range) with the given radii (radius 0: in no list).  Returns (removed ids, per-pass
    counts, radius after pruning, (idx, tr), the final walk)."""
    radius = np.array(radius).copy()
    removed, counts = [], []
    for _ in range(max_passes):
        idx, tr = sort(radius)
        wk = walk(uv, conic, opacity, idx, tr, W, H, bias=bias, K=K, truncate=truncate)
        bad = wk.unclear_ids()
        counts.append(int(bad.size))
        if bad.size == 0:
            return np.array(sorted(removed), np.int64), counts, radius, (idx, tr), wk
        removed.extend(int(i) for i in bad)
        radius[bad] = 0
    raise AssertionError(f"prune did not reach a fixed point in {max_passes} passes: {counts}")


# ------------------------------------------------------------------ float32 restatement of the kernels' arithmetic
F32 = np.float32


def _fma(a, b, c):
    """fused multiply-add of float32 operands, emulated through float64 (the product is exact there; rounds twice)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def f32_tile_alpha(uv, conic, op, ids, x0, y0, nx, ny, bias=None):
    """power_coeffs() / power_poly() term by term -> exp2 -> clamps: (alpha [n,P] float32 with 0 = skipped, raw o G, G)"""
    cx, cy = F32(x0 + 7.5), F32(y0 + 7.5)
    ys, xs = np.meshgrid(np.arange(y0, y0 + ny), np.arange(x0, x0 + nx), indexing="ij")
    x = (xs.reshape(-1).astype(F32) - cx)[None, :]
    y = (ys.reshape(-1).astype(F32) - cy)[None, :]
    u, v = uv[ids, 0].astype(F32)[:, None], uv[ids, 1].astype(F32)[:, None]
    cA, cB, cC = (conic[ids, k].astype(F32)[:, None] for k in range(3))
    o = op[ids].astype(F32)[:, None]
    l2e = F32(1.4426950408889634)
    uc, vc = u - cx, v - cy
    tx = _fma(cA, uc, cB * vc)
    ty = _fma(cB, uc, cC * vc)
    q0 = _fma(F32(-0.5) * l2e, _fma(uc, tx, vc * ty), np.log2(o))
    qx, qy = l2e * tx, l2e * ty
    qxx, qxy, qyy = (F32(-0.5) * l2e) * cA, (-l2e) * cB, (F32(-0.5) * l2e) * cC
    pw = _fma(x, qx, q0)
    pw = _fma(y, qy, pw)
    pw = _fma(x * x, qxx, pw)
    pw = _fma(x * y, qxy, pw)
    pw = _fma(y * y, qyy, pw)
    raw = np.exp2(pw).astype(F32)
    raw = np.where(np.isnan(raw), F32(0), np.clip(raw, F32(0), F32(1))).astype(F32)      # v_exp_f32 ... clamp: NaN -> 0
    if bias is None:
        alpha = np.minimum(F32(0.99), raw)
        alpha = np.where(alpha < F32(1.0 / 255.0), F32(0), alpha).astype(F32)
        G = (raw / o).astype(F32)
    else:   # the bias operator: the reference's factored form on dx, dy, skipped when it comes out negative; fma(o, G, bias)
        dx, dy = u - (x + cx), v - (y + cy)
        q = _fma(dx, _fma(cA, F32(0.5) * dx, cB * dy), (cC * (F32(0.5) * dy)) * dy)
        G = np.exp2(-l2e * q).astype(F32)
        alpha = np.minimum(F32(0.99), _fma(o, G, bias[ids].astype(F32)[:, None]))
        alpha = np.where(~(q < 0) & ~(alpha < F32(1.0 / 255.0)), alpha, F32(0)).astype(F32)
        raw = (o * G).astype(F32)
    return alpha, raw, G, (uc, vc, x, y, cA, cB, cC, o)


def f32_forward_backward(uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, dL_dout=None, bias=None, K=0,
                         truncate=False):
    """The kernels' arithmetic in numpy float32: forward (fmaf accumulation), and the backward as the matrix kernels run it --
    T /= 1 - alpha replayed from final_T, dL/dalpha = T cg - (R + T_final bg.g) / (1 - alpha), six moments of dL/dpower about
    the tile centre, the geometry gradients as linear combinations of them.  Returns dict(image, final_T, ncontrib, gs_idx,
    applied = list of [n, P] masks per tile, grads or None)."""
    uv, conic = np.asarray(uv, F32).reshape(-1, 2), np.asarray(conic, F32).reshape(-1, 3)
    op = np.asarray(opacity, F32).reshape(-1)
    f = np.asarray(feature, F32)
    N, C = f.shape
    bs = None if bias is None else np.asarray(bias, F32).reshape(-1)
    idx = np.asarray(idx_sorted).reshape(-1).astype(np.int64)
    tr = np.asarray(tile_range).reshape(-1, 2).astype(np.int64)
    bgv = _bg_vec(bg, C).astype(F32)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    img = np.zeros((C, H, W), F32)
    fT = np.ones((H, W), F32)
    nc = np.zeros((H, W), np.int32)
    gi = np.full((H, W, max(K, 1)), -1, np.int32)
    masks = []
    grads = None
    if dL_dout is not None:
        gim = np.asarray(dL_dout, F32).reshape(C, H, W)
        grads = dict(uv=np.zeros((N, 2), F32), conic=np.zeros((N, 3), F32), opacity=np.zeros(N, F32), feature=np.zeros((N, C), F32),
                     bias=np.zeros(N, F32), abs_uv=np.zeros((N, 2), F32))
    with np.errstate(all="ignore"):
        for tile in range(gx * gy):
            tx_, ty_ = tile % gx, tile // gx
            x0, y0 = tx_ * TILE, ty_ * TILE
            nx, ny = min(W, x0 + TILE) - x0, min(H, y0 + TILE) - y0
            P = nx * ny
            ids = idx[int(tr[tile, 0]):int(tr[tile, 1])]
            n = ids.size
            alpha, raw, G, geo = f32_tile_alpha(uv, conic, op, ids, x0, y0, nx, ny, bs)
            T = np.ones(P, F32)
            F = np.zeros((P, C), F32)
            done = np.zeros(P, bool)
            last = np.zeros(P, np.int32)
            layer = np.zeros(P, np.int64)
            gsl = np.full((P, max(K, 1)), -1, np.int32)
            app_all = np.zeros((n, P), bool)
            for i in range(n):
                if done.all():
                    break
                ok = ~done & (alpha[i] != 0)
                nT = (T * (F32(1) - alpha[i])).astype(F32)
                sat = ok & (nT < F32(0.0001))
                app = ok & ~sat
                wgt = np.where(app, alpha[i] * T, F32(0)).astype(F32)
                F = _fma(wgt[:, None], f[ids[i]][None, :], F)
                T = np.where(app, nT, T)
                last = np.where(app, i + 1, last)
                done |= sat
                app_all[i] = app
                if K > 0:
                    rec = app & (layer < K)
                    if rec.any():
                        r = np.nonzero(rec)[0]
                        gsl[r, layer[r]] = ids[i]
                        layer = layer + rec
                    if truncate:
                        done |= app & (layer >= K)
            masks.append(app_all)
            sl = (slice(y0, y0 + ny), slice(x0, x0 + nx))
            img[(slice(None),) + sl] = _fma(T[:, None], bgv[None, :], F).T.reshape(C, ny, nx)
            fT[sl], nc[sl], gi[sl] = T.reshape(ny, nx), last.reshape(ny, nx), gsl.reshape(ny, nx, -1)
            if grads is None or n == 0:
                continue
            # ---- backward replay, back to front
            uc, vc, x, y, cA, cB, cC, o = geo
            gp_ = gim[(slice(None),) + sl].reshape(C, P)
            Tf = T
            for c0 in range(0, C, CHUNK):
                c1 = min(C, c0 + CHUNK)
                gch = gp_[c0:c1]
                bgd = (Tf * (bgv[c0:c1] @ gch).astype(F32)).astype(F32)
                Tr = Tf.copy()
                R = np.zeros(P, F32)
                for i in range(int(last.max()) - 1, -1, -1):
                    act = (i < last) & (alpha[i] != 0)
                    if not act.any():
                        continue
                    om = (F32(1) - alpha[i]).astype(F32)
                    Tn = np.where(act, Tr / np.where(act, om, F32(1)), Tr).astype(F32)
                    cg = (f[ids[i], c0:c1] @ gch).astype(F32)
                    dLa = np.where(act, _fma(Tn, cg, -((R + bgd) / np.where(act, om, F32(1))).astype(F32)), F32(0)).astype(F32)
                    wgt = np.where(act, alpha[i] * Tn, F32(0)).astype(F32)
                    R = _fma(wgt, cg, R)
                    Tr = Tn
                    gpw = (dLa * raw[i]).astype(F32)
                    xs_, ys_ = x[0], y[0]
                    m0, mx, my = gpw.sum(dtype=F32), (gpw * xs_).sum(dtype=F32), (gpw * ys_).sum(dtype=F32)
                    mxx, mxy, myy = (gpw * (xs_ * xs_)).sum(dtype=F32), (gpw * (xs_ * ys_)).sum(dtype=F32), (gpw * (ys_ * ys_)).sum(dtype=F32)
                    a_, b_, c_, u_, v_ = cA[i, 0], cB[i, 0], cC[i, 0], uc[i, 0], vc[i, 0]
                    sx, sy = _fma(u_, m0, -mx), _fma(v_, m0, -my)                         # sum gpw dx, sum gpw dy
                    sxx = _fma(u_, _fma(u_, m0, F32(-2) * mx), mxx)
                    syy = _fma(v_, _fma(v_, m0, F32(-2) * my), myy)
                    sxy = _fma(u_, _fma(v_, m0, -my), _fma(-v_, mx, mxy))
                    k = ids[i]
                    grads["uv"][k, 0] += -(_fma(a_, sx, b_ * sy))
                    grads["uv"][k, 1] += -(_fma(c_, sy, b_ * sx))
                    grads["conic"][k, 0] += F32(-0.5) * sxx
                    grads["conic"][k, 1] += -sxy
                    grads["conic"][k, 2] += F32(-0.5) * syy
                    grads["opacity"][k] += (dLa * G[i]).sum(dtype=F32)
                    grads["bias"][k] += dLa.sum(dtype=F32)
                    grads["feature"][k, c0:c1] += (gch @ wgt).astype(F32)
                    dxs, dys = (u_ - xs_).astype(F32), (v_ - ys_).astype(F32)
                    grads["abs_uv"][k, 0] += np.abs(gpw * -(_fma(a_, dxs, b_ * dys))).sum(dtype=F32)
                    grads["abs_uv"][k, 1] += np.abs(gpw * -(_fma(c_, dys, b_ * dxs))).sum(dtype=F32)
    return dict(image=img, final_T=fT, ncontrib=nc, gs_idx=gi, applied=masks, grads=grads)


def worst_ratio(got, ref, comp):
    """max over the elements of |got - ref| / comp (0 / 0 counts as 0; an error where the companion is 0 as infinite)"""
    err = np.abs(np.asarray(got, np.float64).reshape(-1) - np.asarray(ref, np.float64).reshape(-1))
    c = np.asarray(comp, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / c)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------ the scenes of the strict compositing tests
@dataclasses.dataclass
class Scene:
    name: str
    W: int
    H: int
    N: int
    uv: np.ndarray          # operands of the blend (float32)
    conic: np.ndarray
    opacity: np.ndarray
    sort_uv: np.ndarray     # operands of the sort (clean geometry)
    depth: np.ndarray
    radius: np.ndarray      # after culling and pruning
    tiles: np.ndarray
    idx: np.ndarray
    tr: np.ndarray
    culled: np.ndarray      # ids taken out to empty a tile
    pruned: np.ndarray      # ids taken out because a decision was unclear
    passes: list
    bias: Optional[np.ndarray] = None


def _reaches_tile(uv, radius, tx, ty):
    """Gaussians whose tile rectangle (test helper of the sort: (c -+ r) / 16 truncated) contains tile (tx, ty)"""
    r = radius.reshape(-1).astype(np.float64)
    x0, x1 = np.trunc((uv[:, 0] - r) / TILE), np.trunc((uv[:, 0] + r + TILE - 1.0) / TILE)
    y0, y1 = np.trunc((uv[:, 1] - r) / TILE), np.trunc((uv[:, 1] + r + TILE - 1.0) / TILE)
    return (r > 0) & (np.maximum(x0, 0) <= tx) & (tx < x1) & (np.maximum(y0, 0) <= ty) & (ty < y1)


def _finish(o, name, W, H, uv, conic, op, G, radius, culled, bias=None):
    rdt, tl = G["radius"].dtype, G["tiles"]
    live_tiles = lambda r: np.where(r.reshape(-1) == 0, 0, tl.reshape(-1)).reshape(tl.shape).astype(tl.dtype)   # radius 0: no tile
    sort = lambda r: o.sort_gaussian(G["uv"], G["depth"], W, H, r.astype(rdt), live_tiles(r))
    pruned, passes, radius, (idx, tr), _ = prune(uv, conic, op, G["depth"], radius, tl, W, H, sort, bias=bias)
    return Scene(name, W, H, uv.shape[0], uv, conic, op, G["uv"], G["depth"], radius.astype(rdt), live_tiles(radius), idx, tr,
                 np.asarray(culled, np.int64), pruned, passes, bias)


def opaque_scene(o, bias=False):
    """the "opaque" scene of test_gpu_alpha_blending_points_backward.py from the oracle's geometry: 1500 Gaussians at 100 x 60,
    40 % of them in one disc, every Gaussian within 8 px of the disc's densest spot at opacity 0.99; the Gaussians that reach
    the top right tile are culled (radius 0: in no list), so the scene has an empty tile.  bias: the same operands with a
    seeded opacity bias in [-0.05, 0.1] (pruned for the bias operator's decisions)."""
    from splatter_a_video_amd.synth import make_scene
    from test_gpu_parity import oracle_geometry
    N, W, H = 1500, 100, 60
    sc = make_scene(N, W, H, seed=21, clustered=0.4, cluster_area=0.03, blobs=1)
    # The seed saturates single pixels only.  A wall of 64 splats (sigma 5 px, opacity 0.9, in front of everything: 16 about the
    # centre of each 8x8 block of tile (3, 2)) makes that tile saturate entirely, well before the end of its list.
    rng = np.random.default_rng(78)
    probe, _ = o.project_point_ortho_forward(np.array([[-0.5, -0.5, 0.5], [0.5, 0.5, 0.5]], np.float32), sc.extr, W, H, 0.01)
    ax, ay = float(probe[1, 0] - probe[0, 0]), float(probe[1, 1] - probe[0, 1])          # pixels per world unit
    bx, by = float(probe[0, 0]) + 0.5 * ax, float(probe[0, 1]) + 0.5 * ay                # pixel of the world origin
    k = np.arange(64)
    wu = 48 + 3.5 + 8 * (k % 2) + rng.uniform(-0.5, 0.5, 64)
    wv = 32 + 3.5 + 8 * ((k // 2) % 2) + rng.uniform(-0.5, 0.5, 64)
    wall = np.stack([(wu - bx) / ax, (wv - by) / ay, 0.02 + 0.0009 * k], 1).astype(np.float32)
    sc.xyz = np.concatenate([sc.xyz, wall])
    sc.phase = np.concatenate([sc.phase, np.zeros(64, np.float32)])
    sc.scale = np.concatenate([sc.scale, np.tile(np.array([[5.0 / abs(ax), 5.0 / abs(ay), 0.01]], np.float32), (64, 1))])
    sc.rotate = np.concatenate([sc.rotate, np.tile(np.array([[1, 0, 0, 0]], np.float32), (64, 1))])
    sc.opacity = np.concatenate([sc.opacity, np.full((64, 1), 0.9, np.float32)])
    sc.shs = np.concatenate([sc.shs, np.zeros((64,) + sc.shs.shape[1:], np.float32)])
    sc.N = N = N + 64
    G = oracle_geometry(o, sc)
    assert G["vis"].all()
    u = G["uv"]
    assert np.abs(u[-64:, 0] - wu).max() < 1e-3 and np.abs(u[-64:, 1] - wv).max() < 1e-3
    hist, xe, ye = np.histogram2d(u[:1500, 0], u[:1500, 1], bins=[W // 4, H // 4], range=[[0, W], [0, H]])
    ix, iy = np.unravel_index(np.argmax(hist), hist.shape)
    hx, hy = int(xe[ix] + 2), int(ye[iy] + 2)
    op = sc.opacity.copy()
    op[(u[:, 0] - hx) ** 2 + (u[:, 1] - hy) ** 2 < 64] = np.float32(0.99)
    reach = _reaches_tile(u.astype(np.float64), G["radius"], (W - 1) // TILE, 0)
    radius = np.where(reach, 0, G["radius"].reshape(-1)).reshape(G["radius"].shape)
    b = np.random.default_rng(77).uniform(-0.05, 0.1, size=(N, 1)).astype(np.float32) if bias else None
    return _finish(o, "opaque_100x60" + ("_bias" if bias else ""), W, H, G["uv"], G["conic"], op, G, radius, np.nonzero(reach)[0], b)


def hard_scene(o):
    """the operands of test_gpu_forward_poly_matrix._hard (opacity 0 and 1e-30, needle conics above 1e4, splats on pixel and
    tile centres, NaN / inf conic and uv in mid-list), lists from the clean geometry.  The centre alphas that sit ON 1/255 (and
    one float32 step beside it) are undecidable by construction: they are moved to a relative 5e-5 and 7e-5 beside it, on both
    sides (the margin S e_alpha at a splat centre of this scene is below that)."""
    from test_gpu_forward_poly_matrix import _hard
    W, H, N, G, uv, conic, op = _hard(o)
    uv, conic, op = uv.copy(), conic.copy(), op.copy()
    edge = np.float32(A_MIN)
    op[20:60, 0] = np.array([edge * np.float32(1 + 5e-5), edge * np.float32(1 - 5e-5), edge * np.float32(1 + 7e-5), edge * np.float32(1 - 1e-4),
                             edge * np.float32(1 + 1e-4)] * 8, np.float32)
    # A needle's polynomial has terms of 1e6 .. 1e7 log2 units, so float32 cannot decide alpha >= 1/255 on a pixel centre that lies
    # in a band beside the needle's axis (relative error of alpha up to 0.5).  Such a needle is turned in steps of 0.1 rad until
    # no pixel centre of the image lies in its band; the conic keeps its eigenvalues (3e4 and 0.02).
    ang = np.random.default_rng(6).uniform(0, np.pi, size=40)
    big, small = 3e4, 0.02
    for k in range(40):
        for turn in range(64):
            cs, sn = np.cos(ang[k] + 0.1 * turn), np.sin(ang[k] + 0.1 * turn)
            c = np.array([big * cs * cs + small * sn * sn, (big - small) * cs * sn, big * sn * sn + small * cs * cs], np.float32)
            if alpha_decisions_clear(uv[60 + k, 0], uv[60 + k, 1], c[0], c[1], c[2], op[60 + k, 0], W, H):
                break
        else:
            raise AssertionError(f"needle {k}: no clear angle")
        assert turn > 0 or np.array_equal(c, conic[60 + k]), "the needles of test_gpu_forward_poly_matrix._hard"
        conic[60 + k] = c
    assert float(np.abs(conic[60:100]).max()) > 1e4
    return _finish(o, "hard_64x48", W, H, uv, conic, op, G, G["radius"].copy(), [])


_SCENES = {}


def scene(o, name) -> Scene:
    """the scenes by name, built once per session: opaque_100x60, opaque_100x60_bias, hard_64x48"""
    if name not in _SCENES:
        _SCENES[name] = dict(opaque_100x60=lambda: opaque_scene(o), opaque_100x60_bias=lambda: opaque_scene(o, bias=True),
                             hard_64x48=lambda: hard_scene(o))[name]()
    return _SCENES[name]


_WALKS = {}


def scene_walk(sc: Scene, K=0, truncate=False) -> Walk:
    """the float64 walk of a scene, once per (scene, K, truncation) and session"""
    key = (sc.name, K, truncate)
    if key not in _WALKS:
        _WALKS[key] = walk(sc.uv, sc.conic, sc.opacity, sc.idx, sc.tr, sc.W, sc.H, bias=sc.bias, K=K, truncate=truncate)
    return _WALKS[key]


def coverage(sc: Scene, wk: Walk):
    """facts about a walk that the tests assert: list lengths, empty tiles, long lists walked to their end, pixels that stop
    early, tiles that saturate entirely, the longest run of applied entries of one 4x4 quarter (whole list, and within 64
    consecutive list positions: a staged super-batch of the quarter-list kernels)"""
    n = (sc.tr[:, 1] - sc.tr[:, 0]).astype(int)
    long_end = [t.tile for t in wk.tiles if t.nlist > 256 and t.ids.size == t.nlist and bool((~t.stopped).any())]
    early = int(sum(int(t.stopped.sum()) for t in wk.tiles))
    full_sat = [t.tile for t in wk.tiles if t.nlist > 0 and bool(t.stopped.all()) and t.ids.size < t.nlist]
    qmax = q64 = 0
    for t in wk.tiles:
        if t.ids.size == 0:
            continue
        ys, xs = np.meshgrid(np.arange(t.ny), np.arange(t.nx), indexing="ij")
        quarter = ((ys // 4) * 4 + xs // 4).reshape(-1)
        for q in np.unique(quarter):
            hit = t.applied[:, quarter == q].any(1).astype(int)
            qmax = max(qmax, int(hit.sum()))
            c = np.concatenate([[0], np.cumsum(hit)])
            w = min(64, hit.size)
            q64 = max(q64, int((c[w:] - c[:-w]).max()))
    return dict(lengths=n, empty=int((n == 0).sum()), long_to_end=long_end, stopped_pixels=early, saturated_tiles=full_sat,
                quarter_applied=qmax, quarter_applied_64=q64)
