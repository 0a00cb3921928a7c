"""gs.alpha_blending_points(differentiable=True, ordered=True) (splat_alpha_blending_points_backward_ordered, csrc/query.hip): the
backward of the sparse compositing without a float atomic.

Values: against the dense route of tests/test_gpu_alpha_blending_points_backward.py (`_reference`) with that module's bound,
element-wise 2 x (2e-3 |ref| + 1e-4 max |ref|); every case asserts its coverage from corner_ncontrib and tile_range as that module
does.  Bits: on a crowded case (thousands of addends per Gaussian) every gradient is torch.equal run to run, on a side stream
and under the deterministic flag -- the contract of the ordered entry.  Whether the atomic route differs between runs on the
same case is printed, not asserted (it may happen not to)."""
import numpy as np
import pytest
import torch

import dptr.gs as gs
from splatter_a_video_amd import _lib as L
from test_gpu_alpha_blending_points import _query_points, _scene, _t
from test_gpu_alpha_blending_points_backward import (GRAD_NAMES, _assert_coverage, _assert_grads, _coverage, _geom, _integer_pixels,
                                                     _opaque_scene, _reference)

pytestmark = pytest.mark.gpu

WIDE = 300          # crosses the kernel's channel chunk (256 channels per launch)


def _leaves(geom, feat, need=(True, True, True, True)):
    ts = [t.detach().clone() for t in geom[:3]] + [feat.detach().clone()]
    return [t.requires_grad_(True) if n else t for t, n in zip(ts, need)]


def _ordered(geom, feat, bg, pts, g, need=(True, True, True, True), ordered=True, corners=True):
    _, _, _, idx, tr, N, W, H = geom
    uv, conic, op, f = _leaves(geom, feat, need)
    res = gs.alpha_blending_points(uv, conic, op, f, idx, tr, bg, W, H, _t(pts), return_corners=corners, differentiable=True,
                                   ordered=ordered)
    out, cn = (res[0], res[2]) if corners else (res, None)
    out.backward(g)
    return out.detach(), cn, (uv.grad, conic.grad, op.grad, f.grad)


def _compare(name, C, bg, pts, seed, opacity_grad=True):
    geom = _geom(name)
    N = geom[5]
    rng = np.random.default_rng(seed)
    feat = _t(rng.uniform(-1, 1, size=(N, C)))
    g = _t(rng.normal(size=(len(pts), C)))
    ref_val, S, ref_grads = _reference(geom, feat, bg, pts, g, opacity_grad)
    out, cn, grads = _ordered(geom, feat, bg, pts, g, (True, True, opacity_grad, True))
    tol = 1e-5 * (1 + S) + 1e-4 * ref_val.abs()
    assert bool(((out.double() - ref_val).abs() <= tol).all())
    _assert_grads(grads, ref_grads, f"ordered {name} C={C} bg={bg}")
    # the forward that does not walk weightless corners feeds the same backward
    _, _, grads_live = _ordered(geom, feat, bg, pts, g, (True, True, opacity_grad, True), corners=False)
    for a, b in zip(grads, grads_live):
        assert (a is None and b is None) or torch.equal(a, b)
    assert any(float(t.abs().max()) > 0 for t in ref_grads if t is not None)
    return _coverage(geom, pts, cn), grads


def _points(name, kind, seed):
    W, H = _geom(name)[6:]
    if kind == "integer":
        return _integer_pixels(name, seed)
    pts = _query_points(W, H, seed=seed)
    if name == "opaque_100x60":
        hx, hy = _opaque_scene()[1]
        pts = np.concatenate([pts, np.array([[hx + 0.5, hy + 0.25], [hx - 0.875, hy + 0.5]], np.float32)])
    return np.concatenate([pts, pts[[1, 4, 9, 14, 16, 20, 36, 41]], pts[[4, 9]]])       # repeats: sums over queries


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("C", [1, 3, 5, WIDE])
@pytest.mark.parametrize("kind", ["subpixel", "integer"])
@pytest.mark.parametrize("name", ["64_32x32", "1500_100x60", "opaque_100x60"])
def test_ordered_backward_matches_the_dense_route(name, kind, C):
    pts = _points(name, kind, seed=C)
    cov, _ = _compare(name, C, 0.75 if C == 3 else 0.0, pts, seed=100 * C + len(name))
    _assert_coverage(name, cov)


def test_opacity_detached():
    name, C = "opaque_100x60", 3
    cov, grads = _compare(name, C, 0.75, _points(name, "subpixel", 3), seed=31, opacity_grad=False)
    assert grads[2] is None and all(grads[k] is not None for k in (0, 1, 3))
    _assert_coverage(name, cov)


def test_only_the_feature_requires_grad():
    name, C = "1500_100x60", 5
    geom = _geom(name)
    pts = _points(name, "subpixel", 5)
    rng = np.random.default_rng(77)
    feat = _t(rng.uniform(-1, 1, size=(geom[5], C)))
    g = _t(rng.normal(size=(len(pts), C)))
    _, _, ref_grads = _reference(geom, feat, 0.0, pts, g)
    out, cn, grads = _ordered(geom, feat, 0.0, pts, g, (False, False, False, True))
    assert grads[0] is None and grads[1] is None and grads[2] is None
    _assert_grads((None, None, None, grads[3]), (None, None, None, ref_grads[3]), "ordered, feature only")
    _assert_coverage(name, _coverage(geom, pts, cn))


def test_corners_on_an_empty_list_add_nothing():
    geom = _scene("left_half_128x64")
    N, W, H = geom[5:]
    feat = _t(np.random.default_rng(4).uniform(-1, 1, size=(N, 3)))
    pts = np.concatenate([_query_points(W, H, seed=3),
                          np.array([[W - 8.5, H // 2 + 0.25], [W - 3, 7], [W - 1, H - 1], [W - 20, 30], [W - 0.5, 20]], np.float32)])
    g = _t(np.random.default_rng(5).normal(size=(len(pts), 3)))
    _, _, ref_grads = _reference(geom, feat, 0.75, pts, g)
    out, cn, grads = _ordered(geom, feat, 0.75, pts, g)
    assert _coverage(geom, pts, cn)[2] >= 5
    _assert_grads(grads, ref_grads, "ordered, empty lists")


def test_more_than_64_live_corners_in_one_tile():
    """a 9 x 9 grid of quarter-pixel points inside the tile of the opaque scene's dense spot: 225 live corners for one owner"""
    name = "opaque_100x60"
    geom = _geom(name)
    N, W, H = geom[5:]
    hx, hy = _opaque_scene()[1]
    tx, ty = min(hx // 16, (W - 8) // 16), min(hy // 16, (H - 8) // 16)
    q = 0.25 * np.arange(9, dtype=np.float32)
    pts = np.stack(np.meshgrid(tx * 16 + 4 + q, ty * 16 + 4 + q), -1).reshape(-1, 2).astype(np.float32)
    # the live corners, counted from the points: inside the image, nonzero weight -- all of them in tile (tx, ty)
    x0, y0 = np.floor(pts[:, 0]), np.floor(pts[:, 1])
    cx, cy = np.stack([x0, x0 + 1, x0, x0 + 1], 1), np.stack([y0, y0, y0 + 1, y0 + 1], 1)
    wx, wy = np.stack([x0 + 1 - pts[:, 0], pts[:, 0] - x0] * 2, 1), np.stack([y0 + 1 - pts[:, 1]] * 2 + [pts[:, 1] - y0] * 2, 1)
    live = (cx <= W - 1) & (cy <= H - 1) & (wx * wy != 0)
    assert (cx[live] // 16 == tx).all() and (cy[live] // 16 == ty).all()
    assert live.sum() == 225 > 64
    rng = np.random.default_rng(9)
    feat = _t(rng.uniform(-1, 1, size=(N, 3)))
    g = _t(rng.normal(size=(len(pts), 3)))
    _, _, ref_grads = _reference(geom, feat, 0.75, pts, g)
    out, cn, grads = _ordered(geom, feat, 0.75, pts, g)
    applied = int((live & (cn.cpu().numpy() > 0)).sum())
    print(f"live corners in tile ({tx}, {ty}): {int(live.sum())}, with applied entries: {applied}")
    assert applied > 64
    _assert_grads(grads, ref_grads, "ordered, 225 corners in one tile")


# ---------------------------------------------------------------- bits
def test_crowded_gradients_are_bit_reproducible():
    name, C, Q = "1500_100x60", 3, 2048
    geom = _geom(name)
    N, W, H = geom[5:]
    rng = np.random.default_rng(123)
    pts = (np.array([32.0, 16.0]) + rng.uniform(0.0, 16.0, size=(Q, 2))).astype(np.float32)      # inside a 16 x 16 region
    assert pts[:, 0].min() >= 32 and pts[:, 0].max() <= 48 and pts[:, 1].min() >= 16 and pts[:, 1].max() <= 32
    assert ((pts != np.floor(pts)).any(1)).all()
    feat = _t(rng.uniform(-1, 1, size=(N, C)))
    g = _t(rng.normal(size=(Q, C)))
    runs = [_ordered(geom, feat, 0.75, pts, g)[2] for _ in range(5)]
    assert all(float(t.abs().max()) > 0 for t in runs[0])
    for r in runs[1:]:
        for n, a, b in zip(GRAD_NAMES, runs[0], r):
            assert torch.equal(a, b), f"d{n} differs between two runs"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _ordered(geom, feat, 0.75, pts, g)[2]
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    L.set_deterministic(True)
    try:
        flagged = _ordered(geom, feat, 0.75, pts, g)[2]
    finally:
        L.set_deterministic(False)
    for n, a, b, c in zip(GRAD_NAMES, runs[0], on_side, flagged):
        assert torch.equal(a, b), f"d{n} differs on a side stream"
        assert torch.equal(a, c), f"d{n} differs under the deterministic flag"
    # the ordered sums are the atomic route's sums in another order
    atomic = [_ordered(geom, feat, 0.75, pts, g, ordered=False)[2] for _ in range(3)]
    _assert_grads(runs[0], [t.double() for t in atomic[0]], "ordered against atomic, crowded")
    differs = any(not torch.equal(a, b) for r in atomic[1:] for a, b in zip(atomic[0], r))
    print(f"crowded case: the atomic route differs between runs: {differs}")


# ---------------------------------------------------------------- refusals
def test_ordered_needs_differentiable():
    geom = _geom("64_32x32")
    uv, conic, op, idx, tr, N, W, H = geom
    feat = torch.ones(N, 3, device="cuda")
    with pytest.raises(ValueError, match="differentiable"):
        gs.alpha_blending_points(uv, conic, op, feat, idx, tr, 0.0, W, H, _t(_integer_pixels("64_32x32", 1)), ordered=True)


def test_ordered_needs_the_pair_map_in_the_forward():
    geom = _geom("64_32x32")
    _, _, _, idx, tr, N, W, H = geom
    uv, conic, op, f = _leaves(geom, torch.ones(N, 3, device="cuda"))
    with pytest.raises(ValueError, match="pair map"):
        gs.alpha_blending_points(uv, conic, op, f, idx.clone(), tr, 0.0, W, H, _t(_integer_pixels("64_32x32", 1)),
                                 differentiable=True, ordered=True)
    assert all(t.grad is None for t in (uv, conic, op, f))
