"""gs.alpha_blending_points(differentiable=True) (splat_alpha_blending_points_backward, csrc/query.hip) against the project's own
dense route on the GPU: F.grid_sample(gs.alpha_blending(...)[None], grid, align_corners=True) with the same upstream gradient.

Tolerances, the project's: values atol 1e-5 (1 + S) + rtol 1e-4 (S = the same sample of a dense render of |feature|, as in
test_gpu_alpha_blending_points.py); gradients element-wise 2 x (2e-3 |ref| + 1e-4 max |ref|) -- twice the project's gradient
criterion, because both routes carry it against the exact value.  The reference samples the float32 image in float64 (the
bilinear weights of the reference are then exact for points on eighths, like the kernel's).  A point that is not finite or
lies beyond 1e6 contributes nothing by definition; the reference's grid holds (-10, -10) in its place, so that the comparison
does not rest on how grid_sample treats a non-finite coordinate, and a separate test pins "nothing" for those points alone.

Every comparison asserts its own coverage from corner_ncontrib and tile_range: corners whose pixel stopped early (last below the
list length), corners with last >= 65 (more than one 64-entry block), corners on an empty list."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dptr.gs as gs
from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import losses
from splatter_a_video_amd.synth import make_scene
from splatter_a_video_amd.tracks import TrackTargets, frame_weights
from test_gpu_alpha_blending_points import _query_points, _scene, _t

pytestmark = pytest.mark.gpu

GRAD_NAMES = ("uv", "conic", "opacity", "feature")
WORST = {"ratio": 0.0}          # the largest |got - ref| / bound over the gradient comparisons of this module


@functools.lru_cache(maxsize=None)
def _opaque_scene():
    """1500 Gaussians at 100 x 60, 40 % of them in one disc, and every Gaussian within 8 px of the disc's densest pixel at
    opacity 0.99: pixels there stop early.  Returns (geometry, (hx, hy) = that pixel)."""
    N, W, H = 1500, 100, 60
    sc = make_scene(N, W, H, seed=21, clustered=0.4, cluster_area=0.03, blobs=1)
    uv, depth, conic, radius, tiles = gs.preprocess_ortho(_t(sc.xyz), _t(sc.scale), _t(sc.rotate), _t(sc.extr), W, H, nearest=0.01)
    u = uv.cpu().numpy()
    hist, xe, ye = np.histogram2d(u[:, 0], u[:, 1], bins=[W // 4, H // 4], range=[[0, W], [0, H]])
    bx, by = np.unravel_index(np.argmax(hist), hist.shape)
    hx, hy = int(xe[bx] + 2), int(ye[by] + 2)
    op = sc.opacity.copy()
    near = (u[:, 0] - hx) ** 2 + (u[:, 1] - hy) ** 2 < 64
    assert near.sum() >= 50
    op[near] = 0.99
    idx, tr = gs.sort_gaussian(uv, depth, W, H, radius, tiles)
    return (uv, conic, _t(op), idx, tr, N, W, H), (hx, hy)


def _geom(name):
    return _opaque_scene()[0] if name == "opaque_100x60" else _scene(name)


def _integer_pixels(name, seed, n=40):
    """unique integer query pixels: random ones, the image corners, and on the opaque scene a 5 x 5 window on the dense spot"""
    W, H = _geom(name)[6:]
    rng = np.random.default_rng(seed)
    pix = set(rng.choice(W * H, size=min(n, W * H), replace=False).tolist()) | {0, W - 1, (H - 1) * W, H * W - 1}
    if name == "opaque_100x60":
        hx, hy = _opaque_scene()[1]
        pix |= {y * W + x for y in range(hy - 2, hy + 3) for x in range(hx - 2, hx + 3) if 0 <= x < W and 0 <= y < H}
    pix = np.array(sorted(pix))
    return np.stack([pix % W, pix // W], 1).astype(np.float32)


def _leaves(geom, feat, opacity_grad=True):
    uv, conic, op = (t.detach().clone().requires_grad_(True) for t in geom[:3])
    if not opacity_grad:
        op.requires_grad_(False)
    return uv, conic, op, feat.detach().clone().requires_grad_(True)


def _reference(geom, feat, bg, pts, g, opacity_grad=True):
    """the dense route: (values [Q, C] float64, S, the four gradients)"""
    _, _, _, idx, tr, N, W, H = geom
    uv, conic, op, f = _leaves(geom, feat, opacity_grad)
    img = gs.alpha_blending(uv, conic, op, f, idx, tr, bg, W, H)
    p = np.asarray(pts, np.float64).copy()
    bad = ~np.isfinite(p).all(1) | (np.abs(np.nan_to_num(p, nan=0.0, posinf=1e30, neginf=-1e30)).max(1) > 1e6)
    p[bad] = -10.0                                       # "contributes nothing", independent of grid_sample's NaN handling
    grid = torch.tensor(np.stack([2 * p[:, 0] / (W - 1) - 1, 2 * p[:, 1] / (H - 1) - 1], -1), device="cuda")[None, :, None, :]
    samp = lambda im: F.grid_sample(im[None].double(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, :, 0].T
    val = samp(img)
    val.backward(g.double())
    with torch.no_grad():
        S = samp(gs.alpha_blending(uv, conic, op, f.abs(), idx, tr, abs(bg), W, H))
    return val.detach(), S, (uv.grad, conic.grad, op.grad, f.grad)


def _sparse(geom, feat, bg, pts, g, opacity_grad=True, corners=True):
    """corners=False: nobody reads the corner maps, the forward walks only the corners that carry weight (cn is None)"""
    _, _, _, idx, tr, N, W, H = geom
    uv, conic, op, f = _leaves(geom, feat, opacity_grad)
    res = gs.alpha_blending_points(uv, conic, op, f, idx, tr, bg, W, H, _t(pts), return_corners=corners, differentiable=True)
    out, cT, cn = res if corners else (res, None, None)
    assert out.requires_grad and (not corners or (not cT.requires_grad and not cn.requires_grad))
    out.backward(g)
    return out.detach(), cn, (uv.grad, conic.grad, op.grad, f.grad)


def _coverage(geom, pts, cn):
    """(early, deep, empty): corners with a nonzero bilinear weight inside the image whose pixel stopped below its list length,
    whose last applied entry sits past the first 64-entry block, whose tile list is empty"""
    tr, W, H = geom[4], geom[6], geom[7]
    p = np.asarray(pts, np.float32)
    with np.errstate(invalid="ignore"):
        x0, y0 = np.floor(p[:, 0]), np.floor(p[:, 1])
        cx = np.stack([x0, x0 + 1, x0, x0 + 1], 1)
        cy = np.stack([y0, y0, y0 + 1, y0 + 1], 1)
        wx = np.stack([x0 + 1 - p[:, 0], p[:, 0] - x0] * 2, 1)
        wy = np.stack([y0 + 1 - p[:, 1]] * 2 + [p[:, 1] - y0] * 2, 1)
        live = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1) & (wx * wy != 0)
    trn = tr.cpu().numpy().reshape(-1, 2)
    gx = (W + 15) // 16
    tile = np.where(live, cy, 0).astype(np.int64) // 16 * gx + np.where(live, cx, 0).astype(np.int64) // 16
    n = (trn[:, 1] - trn[:, 0])[tile]
    last = cn.cpu().numpy()
    assert ((last <= n) | ~live).all()
    return int((live & (last < n)).sum()), int((live & (last >= 65)).sum()), int((live & (n == 0)).sum())


def _assert_grads(got, ref, what):
    worst = 0.0
    for name, a, b in zip(GRAD_NAMES, got, ref):
        assert (a is None) == (b is None), f"{what}: {name}.grad is None on one side only"
        if a is None:
            continue
        assert a.shape == b.shape, (name, a.shape, b.shape)
        a64, b64 = a.double().cpu().numpy().reshape(-1), b.double().cpu().numpy().reshape(-1)
        assert np.isfinite(a64).all(), f"{what}: {name} gradient not finite"
        lim = 2.0 * (2e-3 * np.abs(b64) + 1e-4 * np.abs(b64).max())
        err = np.abs(a64 - b64)
        ratio = float(np.max(err / np.maximum(lim, 1e-300))) if b64.size and np.abs(b64).max() > 0 else float(err.max() > 0 if err.size else 0)
        worst = max(worst, ratio)
        print(f"{what}: d{name} max |ref| {np.abs(b64).max() if b64.size else 0:.3e}, worst err / bound {ratio:.4f}")
        assert (err <= lim).all(), f"{what}: d{name}: {int((err > lim).sum())} of {a64.size} off, worst {ratio:.2f} x the bound"
    WORST["ratio"] = max(WORST["ratio"], worst)
    print(f"largest err / bound so far: {WORST['ratio']:.4f}")


def _compare(name, C, bg, pts, seed, opacity_grad=True):
    geom = _geom(name)
    N = geom[5]
    rng = np.random.default_rng(seed)
    feat = _t(rng.uniform(-1, 1, size=(N, C)))
    g = _t(rng.normal(size=(len(pts), C)))
    ref_val, S, ref_grads = _reference(geom, feat, bg, pts, g, opacity_grad)
    out, cn, grads = _sparse(geom, feat, bg, pts, g, opacity_grad)
    tol = 1e-5 * (1 + S) + 1e-4 * ref_val.abs()
    err = (out.double() - ref_val).abs()
    print(f"{name} C={C} bg={bg}: values max err / tol {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), f"{int((err > tol).sum())} values off"
    _assert_grads(grads, ref_grads, f"{name} C={C} bg={bg}")
    out_live, _, grads_live = _sparse(geom, feat, bg, pts, g, opacity_grad, corners=False)
    assert torch.equal(out_live, out), "the forward that skips weightless corners must give the same bits"
    _assert_grads(grads_live, ref_grads, f"{name} C={C} bg={bg} (weightless corners not walked)")
    assert any(float(t.abs().max()) > 0 for t in ref_grads if t is not None)
    return _coverage(geom, pts, cn), grads


def _assert_coverage(name, cov):
    early, deep, empty = cov
    print(f"{name}: corners early-stopped {early}, last >= 65 {deep}, on an empty list {empty}")
    if name == "opaque_100x60":
        assert early >= 1 and deep >= 1
    if name == "1500_100x60":
        assert deep >= 1
    if name == "left_half_128x64":
        assert empty >= 1


# ---------------------------------------------------------------- (a) integer pixels, unique: the track loss's case
@pytest.mark.parametrize("bg", [0.0, 0.75])
@pytest.mark.parametrize("C", [1, 3, 19, 70, 300])
@pytest.mark.parametrize("name", ["64_32x32", "1500_100x60", "opaque_100x60"])
def test_integer_pixels_match_the_dense_route(name, C, bg):
    pts = _integer_pixels(name, seed=C)
    assert len(np.unique(pts, axis=0)) == len(pts)
    cov, _ = _compare(name, C, bg, pts, seed=100 * C + len(name))
    _assert_coverage(name, cov)


# ---------------------------------------------------------------- (b) points on eighths, some of them twice
@pytest.mark.parametrize("C,bg", [(3, 0.75), (70, 0.0)])
@pytest.mark.parametrize("name", ["1500_100x60", "opaque_100x60", "left_half_128x64"])
def test_points_on_eighths_match_the_dense_route(name, C, bg):
    W, H = _geom(name)[6:]
    pts = _query_points(W, H, seed=C)
    if name == "opaque_100x60":
        hx, hy = _opaque_scene()[1]
        pts = np.concatenate([pts, np.array([[hx + 0.5, hy + 0.25], [hx - 0.875, hy + 0.5]], np.float32)])
    pts = np.concatenate([pts, pts[[1, 4, 9, 14, 16, 20, 36, 41]], pts[[4, 9]]])       # repeats: sums over queries
    cov, _ = _compare(name, C, bg, pts, seed=7 * C + len(name))
    _assert_coverage(name, cov)


def test_points_outside_or_not_finite_leave_every_gradient_untouched():
    geom = _geom("1500_100x60")
    N, W, H = geom[5:]
    nan, inf = float("nan"), float("inf")
    pts = np.array([[-1, 2], [W, 3], [2, H], [-5, -5], [W + 2.5, H + 1], [1e9, 1e9], [1e9, 2], [-1e9, 3], [4, -1e9], [3e38, 1],
                    [nan, 3], [3, nan], [nan, nan], [inf, 2], [2, -inf], [-inf, inf]], np.float32)
    feat = _t(np.random.default_rng(3).uniform(-1, 1, size=(N, 5)))
    out, cn, grads = _sparse(geom, feat, 0.75, pts, torch.ones(len(pts), 5, device="cuda"))
    assert float(out.abs().max()) == 0          # ((-1, 2) and (W, 3) touch an in-image corner with weight 0: it is walked, it adds nothing)
    for name, t in zip(GRAD_NAMES, grads):
        assert t is not None and float(t.abs().max()) == 0, name


def test_forward_of_the_live_corners_reports_the_same_values_and_maps():
    """splat_alpha_blending_points_forward_live against splat_alpha_blending_points_forward: out bit-equal, the corner maps equal
    where a corner carries weight and 0 where it does not"""
    geom = _geom("1500_100x60")
    uv, conic, op, idx, tr, N, W, H = geom
    pts = np.concatenate([_query_points(W, H, seed=2), _integer_pixels("1500_100x60", seed=2)])
    for C in (3, 300):
        feat = _t(np.random.default_rng(C).uniform(-1, 1, size=(N, C)))
        res = []
        for fn in (L.lib().splat_alpha_blending_points_forward, L.lib().splat_alpha_blending_points_forward_live):
            out = torch.full((len(pts), C), 7.0, device="cuda")
            cT = torch.full((len(pts), 4), 7.0, device="cuda")
            cn = torch.full((len(pts), 4), 7, dtype=torch.int32, device="cuda")
            L.check(fn(N, C, L.ptr(uv), L.ptr(conic), L.ptr(op), L.ptr(feat), L.ptr(idx), L.ptr(tr), 0.75, W,
                       H, len(pts), L.ptr(_t(pts)), L.ptr(out), L.ptr(cT), L.ptr(cn), L.stream()))
            res.append((out, cT.cpu().numpy(), cn.cpu().numpy()))
        (out_a, T_a, n_a), (out_b, T_b, n_b) = res
        assert torch.equal(out_a, out_b)
        with np.errstate(invalid="ignore"):
            fx, fy = pts[:, 0] - np.floor(pts[:, 0]), pts[:, 1] - np.floor(pts[:, 1])
            wgt = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], 1)
        live = np.nan_to_num(wgt, nan=0.0) != 0
        assert np.array_equal(np.where(live, T_a, 0).view(np.uint32), T_b.view(np.uint32)) and np.array_equal(np.where(live, n_a, 0), n_b)
        assert (~live & (n_a > 0)).sum() >= 100 and (live & (n_a > 0)).sum() >= 100


# ---------------------------------------------------------------- (c) opacity without grad
def test_opacity_without_grad_passes_null():
    name, C, bg = "opaque_100x60", 3, 0.75
    pts = _integer_pixels(name, seed=C)
    cov, grads = _compare(name, C, bg, pts, seed=100 * C + len(name), opacity_grad=False)
    assert grads[2] is None and all(grads[k] is not None for k in (0, 1, 3))      # (the others: compared as in case (a))
    _assert_coverage(name, cov)


# ---------------------------------------------------------------- (d) empty inputs
def test_empty_inputs_give_zero_gradients():
    geom = _geom("left_half_128x64")
    uv0, conic0, op0, idx, tr, N, W, H = geom
    feat = _t(np.random.default_rng(4).uniform(-1, 1, size=(N, 3)))
    # Q = 0
    out, cn, grads = _sparse(geom, feat, 0.5, np.zeros((0, 2), np.float32), torch.zeros(0, 3, device="cuda"))
    assert out.shape == (0, 3) and all(t is not None and float(t.abs().max()) == 0 for t in grads)
    # P = 0: the value is bg times the in-image weights, no gradient to give
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    ntiles = tr.numel() // 2
    pts = _query_points(W, H, seed=0)
    leaves = [z(0, 2).requires_grad_(True), z(0, 3).requires_grad_(True), z(0, 1).requires_grad_(True), z(0, 4).requires_grad_(True)]
    out = gs.alpha_blending_points(*leaves, z(0, dt=torch.int32), z(ntiles, 2, dt=torch.int32), 0.5, W, H, _t(pts), differentiable=True)
    out.sum().backward()
    assert all(t.grad is not None and t.grad.shape == t.shape for t in leaves)
    # the right half is empty: queries there see only the background
    right = np.array([[W - 8.5, H // 2 + 0.25], [W - 3, 7], [W - 1, H - 1], [W - 20, 30], [W - 0.5, 20]], np.float32)
    g = torch.ones(len(right), 3, device="cuda")
    out, cn, grads = _sparse(geom, feat, 0.75, right, g)
    assert int(cn.abs().max()) == 0 and _coverage(geom, right, cn)[2] >= 5
    assert all(float(t.abs().max()) == 0 for t in grads)
    ref_val, _, ref_grads = _reference(geom, feat, 0.75, right, g)
    assert all(float(t.abs().max()) == 0 for t in ref_grads)
    assert float((out.double() - ref_val).abs().max()) <= 1e-6


# ---------------------------------------------------------------- (e) the deterministic flag
def test_deterministic_mode_refuses_the_backward():
    geom = _geom("64_32x32")
    N, W, H = geom[5:]
    feat = torch.ones(N, 3, device="cuda")
    pts = _integer_pixels("64_32x32", seed=1)
    uv, conic, op, f = _leaves(geom, feat)
    out = gs.alpha_blending_points(uv, conic, op, f, geom[3], geom[4], 0.0, W, H, _t(pts), differentiable=True)
    L.set_deterministic(True)
    try:
        with pytest.raises(L.SplatError, match="deterministic"):
            out.sum().backward()
    finally:
        L.set_deterministic(False)
    assert f.grad is None
    out = gs.alpha_blending_points(uv, conic, op, f, geom[3], geom[4], 0.0, W, H, _t(pts), differentiable=True)
    out.sum().backward()                                  # the flag is off again: the backward runs
    assert f.grad is not None and float(f.grad.abs().max()) > 0


# ---------------------------------------------------------------- (f) the track term end to end
@pytest.mark.parametrize("name,C", [("1500_100x60", 3), ("opaque_100x60", 5)])
def test_track_loss_sparse_matches_the_dense_track_term(name, C):
    geom = _geom(name)
    _, _, _, idx, tr, N, W, H = geom
    rng = np.random.default_rng(17 + C)
    track_gs = _t(rng.uniform(-0.9, 0.9, size=(N, C)))
    q = _integer_pixels(name, seed=5, n=300)
    Q = len(q)
    with torch.no_grad():
        img = gs.alpha_blending(geom[0], geom[1], geom[2], track_gs, idx, tr, 0.0, W, H).cpu().numpy()
    qi = q.astype(np.int64)
    t = np.zeros((Q, 4), np.float32)
    off = rng.normal(0, 3.0, size=(Q, 2))
    off[rng.random(Q) < 0.03] *= 20.0                      # outliers for the quantile to drop
    t[:, 0] = (img[0, qi[:, 1], qi[:, 0]] + 1) * W / 2 + off[:, 0]
    t[:, 1] = (img[1, qi[:, 1], qi[:, 0]] + 1) * H / 2 + off[:, 1]
    t[:, 2] = np.where(rng.random(Q) < 0.25, 3.0, -3.0)    # a quarter occluded; logits far from the visibility threshold
    t[:, 3] = -3.0
    tt = TrackTargets.from_reference(q, t, H, W).to("cuda")
    w = frame_weights([3], [7], 50)

    uv, conic, op, f = _leaves(geom, track_gs)
    dense = losses.track_loss(gs.alpha_blending(uv, conic, op.detach(), f, idx, tr, 0.0, W, H)[None, :3], tt, w)
    dense.backward()
    ref = (uv.grad, conic.grad, op.grad, f.grad)
    uv, conic, op, f = _leaves(geom, track_gs)
    sparse = losses.track_loss_sparse(uv, conic, op, f, idx, tr, W, H, tt, w)
    sparse.backward()
    got = (uv.grad, conic.grad, op.grad, f.grad)
    assert got[2] is None and ref[2] is None
    print(f"track term {name}: dense {float(dense):.7f} sparse {float(sparse):.7f}")
    assert float(dense) > 0 and abs(float(sparse) - float(dense)) <= 1e-5 + 1e-4 * abs(float(dense))
    _assert_grads(got, ref, f"track term {name}")
    assert float(f.grad[:, 3:].abs().max()) == 0 if C > 3 else True
