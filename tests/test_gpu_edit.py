"""Appearance editing on the GPU (splatter_a_video_amd/edit.py, csrc/edit.hip) against the project's own dense route:
F.mse_loss(gs.alpha_blending(...).permute(1, 2, 0), target) with autograd w.r.t. ``feature`` only, and a twin of the whole fit
through the existing operators plus torch.optim.Adam.

Tolerances, the project's: image atol 1e-5 + rtol 1e-4; gradients element-wise 2 x (2e-3 |ref| + 1e-4 max |ref|) -- twice the
project's gradient criterion, because both routes carry it against the exact value (as the sparse-compositing tests argue); the
loss within mean(2 |r| d + d^2), d = 1e-5 + 1e-4 |out|, r = out - target: what the image tolerance allows the mean square to move.

Scenes: synth.make_scene, 1500 Gaussians at 100 x 60 (no multiple of 16 either way); the Gaussians that would reach the top
right tile have radius 0 (culled: in no list), so every scene has an empty tile.  Every comparison asserts its own coverage from
tile_range and ncontrib: an empty tile, a list longer than two staging batches of the kernel (2 x 64 entries), pixels whose last
contributor lies below their list length."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import gs
from splatter_a_video_amd.edit import AppearanceFit, blend_fit_color, fit_appearance, select_gaussians
from splatter_a_video_amd.renderer import OrthoEnhancedRenderer
from splatter_a_video_amd.synth import make_scene

pytestmark = pytest.mark.gpu

N, W, H = 1500, 100, 60
GX, GY = (W + 15) // 16, (H + 15) // 16
T = GX * GY
BATCH = 64                       # csrc/edit.hip FIT_SB
SCENES = ("plain", "opaque", "clustered")
LR = 0.0025


def _t(a, dtype=np.float32):
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


@functools.lru_cache(maxsize=None)
def _scene(name):
    """frozen geometry of a seeded scene, sorted once with the pair map"""
    if name == "plain":
        sc = make_scene(N, W, H, seed=11)
    elif name == "opaque":      # the "opaque disc" of test_gpu_alpha_blending_points_backward.py: pixels that stop early
        sc = make_scene(N, W, H, seed=21, clustered=0.4, cluster_area=0.03, blobs=1)
    else:
        sc = make_scene(N, W, H, seed=31, clustered=0.5, cluster_area=0.1, blobs=3)
    uv, depth, conic, radius, tiles = gs.preprocess_ortho(_t(sc.xyz), _t(sc.scale), _t(sc.rotate), _t(sc.extr), W, H, nearest=0.01)
    op = sc.opacity.copy()
    u = uv.cpu().numpy()
    if name == "opaque":
        hist, xe, ye = np.histogram2d(u[:, 0], u[:, 1], bins=[W // 4, H // 4], range=[[0, W], [0, H]])
        bx, by = np.unravel_index(np.argmax(hist), hist.shape)
        near = (u[:, 0] - (xe[bx] + 2)) ** 2 + (u[:, 1] - (ye[by] + 2)) ** 2 < 64
        assert near.sum() >= 50
        op[near] = 0.99
    # nothing reaches the top right tile (columns 96 .. 99, rows 0 .. 15): those Gaussians are culled (radius 0: in no list)
    r = radius.cpu().numpy()
    reach = (u[:, 0] + r >= 95.0) & (u[:, 1] - r < 17.0)
    radius = _t(np.where(reach, 0, r), np.int32)
    idx, tr, status = gs.sort_gaussian_capped(uv, depth, W, H, radius, None)
    pm = status.pairmap
    return dict(uv=uv, depth=depth, conic=conic, radius=radius, tiles=tiles, op=_t(op), shs=_t(sc.shs), idx=idx, tr=tr, goff=pm.goff,
                slot=pm.slot_sorted, M=idx.numel())


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(feature [N, 3], target [H, W, 3]): the scene's colours and a seeded random image"""
    s = _scene(name)
    rng = np.random.default_rng(100 + SCENES.index(name))
    return OrthoEnhancedRenderer.colors(s["shs"]), _t(rng.uniform(0.0, 1.0, size=(H, W, 3)))


def _weighted_mse(img, target, pw):
    d2 = (img.permute(1, 2, 0) - target) ** 2
    return F.mse_loss(img.permute(1, 2, 0), target) if pw is None else (pw[..., None] * d2).mean()


@functools.lru_cache(maxsize=None)
def _dense(name, weighted=False):
    """the dense route, once per scene: (image, loss, d loss / d feature, ncontrib)"""
    s = _scene(name)
    feat, target = _inputs(name)
    f = feat.detach().clone().requires_grad_(True)
    img = gs.alpha_blending(s["uv"], s["conic"], s["op"], f, s["idx"], s["tr"], 0.0, W, H)
    loss = _weighted_mse(img, target, _pixel_weight() if weighted else None)
    loss.backward()
    with torch.no_grad():
        _, nc, _ = gs.alpha_blending_enhanced(s["uv"], s["conic"], s["op"], feat, s["idx"], s["tr"], 0.0, W, H, K=1)
    return img.detach(), loss.detach(), f.grad, nc


@functools.lru_cache(maxsize=None)
def _pixel_weight():
    pw = torch.ones(H, W, device="cuda")
    pw[7:41, 20:71] = 0.0            # a rectangle that cuts through tiles
    return pw


def _native(name, feature, target, pw=None, active=None, buffers=None, want_maps=True):
    """one splat_blend_fit_color + loss sum + segment sum: (loss [1], dcolor [N, 4], out, ncontrib, tile_loss, pair_grad)"""
    s = _scene(name)
    tile_loss, pair_grad = buffers if buffers is not None else (torch.zeros(T, device="cuda"), torch.zeros(s["M"], 4, device="cuda"))
    out = torch.full((3, H, W), float("nan"), device="cuda") if want_maps else None
    nc = torch.full((H, W), -7, dtype=torch.int32, device="cuda") if want_maps else None
    blend_fit_color(s["uv"], s["conic"], s["op"], feature, s["idx"], s["tr"], s["slot"], 0.0, W, H, target, tile_loss, pair_grad,
                    pw, active, None, out, nc)
    hist = torch.zeros(3, device="cuda")
    L.check(L.lib().splat_tile_loss_sum(T, L.ptr(tile_loss), L.ptr(hist), 1, L.stream()))
    dcolor = torch.empty(N, 4, device="cuda")
    L.check(L.lib().splat_pair_records_segment_sum(N, 4, L.ptr(pair_grad), L.ptr(s["goff"]), L.ptr(dcolor), L.stream()))
    assert hist[0] == 0 and hist[2] == 0                  # only history[slot] is written
    return hist[1:2], dcolor, out, nc, tile_loss, pair_grad


def _assert_coverage(name, nc):
    s = _scene(name)
    n = (s["tr"][:, 1] - s["tr"][:, 0]).cpu().numpy().reshape(GY, GX)
    assert n[0, GX - 1] == 0 and (n == 0).sum() >= 1, "an empty tile"
    assert n.max() > 2 * BATCH, f"a list longer than two staging batches: longest {n.max()}"
    per_pixel = np.repeat(np.repeat(n, 16, 0), 16, 1)[:H, :W]
    last = nc.cpu().numpy()
    assert (last <= per_pixel).all()
    assert ((last < per_pixel) & (last > 0)).sum() >= 100, "pixels whose last contributor lies below their list length"
    if name == "opaque":     # pixels that stopped: saturated well before the end of a long list
        assert (last < per_pixel // 2).sum() >= 20
    print(f"{name}: lists up to {n.max()}, {(n == 0).sum()} empty tiles, last < n on {(last < per_pixel).sum()} pixels")


def _loss_bound(img, target, pw=None):
    """what the image tolerance allows the mean square to move: mean(2 |r| d + d^2), d = 1e-5 + 1e-4 |out|"""
    out = img.permute(1, 2, 0).double()
    d = 1e-5 + 1e-4 * out.abs()
    b = 2 * (out - target.double()).abs() * d + d * d
    return float((b if pw is None else pw[..., None].double() * b).mean())


def _assert_grad(got, ref, what, rows=None):
    a, b = got.double().cpu().numpy(), ref.double().cpu().numpy()
    assert np.isfinite(a).all()
    lim = 2.0 * (2e-3 * np.abs(b) + 1e-4 * np.abs(b).max())
    err = np.abs(a - b)
    if rows is not None:
        err, lim = err[rows], lim[rows]
    print(f"{what}: max |ref| {np.abs(b).max():.3e}, worst err / bound {float((err / lim).max()):.4f}")
    assert (err <= lim).all(), f"{what}: {int((err > lim).sum())} of {err.size} off, worst {float((err / lim).max()):.2f} x the bound"


def _compare_with_dense(name, weighted):
    feat, target = _inputs(name)
    pw = _pixel_weight() if weighted else None
    img, loss_ref, dfeat_ref, nc_ref = _dense(name, weighted)
    loss, dcolor, out, nc, _, _ = _native(name, feat, target, pw)
    _assert_coverage(name, nc_ref)
    assert torch.equal(nc, nc_ref), "ncontrib must be the forward's"
    assert not torch.isnan(out).any()
    err = (out - img).abs()
    assert (err <= 1e-5 + 1e-4 * img.abs()).all(), f"image: worst {float(err.max()):.3e}"
    assert float(dfeat_ref.abs().max()) > 0
    _assert_grad(dcolor[:, :3], dfeat_ref, f"{name} dcolor")
    assert (dcolor[:, 3] == 0).all()
    bound = _loss_bound(img, target, pw)
    print(f"{name}: loss {float(loss):.8f} dense {float(loss_ref):.8f} |diff| {abs(float(loss) - float(loss_ref)):.3e} bound {bound:.3e}")
    assert abs(float(loss) - float(loss_ref)) <= bound


@pytest.mark.parametrize("name", SCENES)
def test_kernel_against_the_dense_route(gpu, name):
    _compare_with_dense(name, False)


@pytest.mark.parametrize("name", ("plain", "opaque"))
def test_pixel_weight(gpu, name):
    """zeros over a rectangle, ones elsewhere, against the dense route with the weighted loss; the lanes of the border tiles that
    lie outside the 100 x 60 image contribute nothing in either test (the loss and every gradient would be off otherwise)"""
    _compare_with_dense(name, True)
    # a Gaussian seen only under the rectangle gets an exactly zero gradient
    feat, target = _inputs(name)
    _, dcolor, _, _, _, _ = _native(name, feat, target, _pixel_weight())
    _, _, dfeat_ref, _ = _dense(name, True)
    zero = (dfeat_ref == 0).all(1)
    assert (dcolor[zero] == 0).all()


@functools.lru_cache(maxsize=None)
def _selection(name):
    """(selected bool [N], active tiles int32): the Gaussians listed under a disc mask, the tiles whose list holds one"""
    s = _scene(name)
    feat, _ = _inputs(name)
    _, _, gs_idx = gs.alpha_blending_enhanced(s["uv"], s["conic"], s["op"], feat, s["idx"], s["tr"], 0.0, W, H, K=10)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = _t(((xx - 38) ** 2 + (yy - 30) ** 2 < 11 ** 2).astype(np.float32))       # ~ 6 % of the image
    sel = select_gaussians(gs_idx[None], mask, N)
    hit = sel[s["idx"].long()].cpu().numpy()
    tr = s["tr"].cpu().numpy()
    active = np.array([t for t in range(T) if hit[tr[t, 0]:tr[t, 1]].any()], np.int32)
    assert 0 < int(sel.sum()) < N and 0 < active.size < T
    return sel, _t(active, np.int32)


@pytest.mark.parametrize("name", ("plain", "clustered"))
def test_active_tiles(gpu, name):
    s = _scene(name)
    feat0, target = _inputs(name)
    sel, active = _selection(name)
    gen = torch.Generator(device="cuda").manual_seed(3)
    feat1 = feat0.clone()
    feat1[sel] = torch.rand(int(sel.sum()), 3, device="cuda", generator=gen)
    loss_all, dcolor_all, _, nc, _, _ = _native(name, feat1, target)
    _assert_coverage(name, nc)
    # the buffers as an iteration finds them: every tile at the initial colours, then only the active tiles at the new ones
    _, _, _, _, tile_loss, pair_grad = _native(name, feat0, target, want_maps=False)
    before = tile_loss.clone()
    loss_act, dcolor_act, _, _, _, _ = _native(name, feat1, target, active=active, buffers=(tile_loss, pair_grad), want_maps=False)
    inactive = _t(np.setdiff1d(np.arange(T), active.cpu().numpy()), np.int64)
    assert torch.equal(tile_loss[inactive], before[inactive]) and not torch.equal(tile_loss, before)
    assert torch.equal(loss_act, loss_all), "the loss history entry must be bit-equal to the all-tiles call"
    assert torch.equal(dcolor_act[sel], dcolor_all[sel]), "dcolor of the selected Gaussians must be bit-equal"
    # n_active == 0: success, nothing launched
    keep = tile_loss.clone()
    lib = L.lib()
    rc = lib.splat_blend_fit_color(N, 3, L.ptr(s["uv"]), L.ptr(s["conic"]), L.ptr(s["op"]), L.ptr(feat0), L.ptr(s["idx"]),
                                   L.ptr(s["tr"]), L.ptr(s["slot"]), s["M"], 0.0, W, H, L.ptr(target),
                                   L.ptr(None), 0, L.ptr(active), L.ptr(tile_loss), L.ptr(pair_grad), L.ptr(None), L.ptr(None),
                                   L.stream())
    assert rc == 0
    blend_fit_color(s["uv"], s["conic"], s["op"], feat0, s["idx"], s["tr"], s["slot"], 0.0, W, H, target, tile_loss, pair_grad,
                    active_tiles=active[:0])
    torch.cuda.synchronize()
    assert torch.equal(tile_loss, keep)


def _fit(name, selected, **kw):
    s = _scene(name)
    return AppearanceFit(s["uv"], s["depth"], s["conic"], s["radius"], s["tiles"], s["op"], s["shs"], selected, W, H, lr=LR, **kw)


@functools.lru_cache(maxsize=None)
def _edit_target(name):
    """the scene rendered with other SH values on the selected Gaussians"""
    s = _scene(name)
    sel, _ = _selection(name)
    gen = torch.Generator(device="cuda").manual_seed(17)
    shs2 = s["shs"].clone()
    shs2[sel] = s["shs"][sel] + 0.3 * torch.randn(int(sel.sum()), 16, 3, device="cuda", generator=gen)
    img = gs.alpha_blending(s["uv"], s["conic"], s["op"], OrthoEnhancedRenderer.colors(shs2), s["idx"], s["tr"], 0.0, W, H)
    return img.permute(1, 2, 0).contiguous()


def test_reproducibility(gpu):
    sel, _ = _selection("plain")
    target = _edit_target("plain")
    runs = [_fit("plain", sel).run(target, max_iters=12, tol=float("-inf")) for _ in range(2)]
    old = L.deterministic()
    try:
        L.set_deterministic(True)
        runs += [_fit("plain", sel).run(target, max_iters=12, tol=float("-inf")) for _ in range(2)]
    finally:
        L.set_deterministic(old)
    assert L.deterministic() == old
    shs0, losses0, it0 = runs[0]
    assert it0 == 12 and losses0.shape == (12,) and not torch.equal(shs0, _scene("plain")["shs"])
    for shs, losses, it in runs[1:]:
        assert it == it0 and torch.equal(shs, shs0) and torch.equal(losses, losses0)


def _twin(name, sel, target, iters, sh_rows="all"):
    """the same fit through the existing operators and torch.optim.Adam on shs[selected]: (losses, first image)"""
    s = _scene(name)
    idx = torch.nonzero(sel).reshape(-1)
    base = s["shs"][idx].clone()
    param = (base[:, :1] if sh_rows == "dc" else base).clone().requires_grad_(True)
    opt = torch.optim.Adam([param], lr=LR)
    losses, first = [], None
    for _ in range(iters):
        rows = torch.cat([param, base[:, 1:]], 1) if sh_rows == "dc" else param
        shs = s["shs"].index_copy(0, idx, rows)
        img = gs.alpha_blending(s["uv"], s["conic"], s["op"], OrthoEnhancedRenderer.colors(shs), s["idx"], s["tr"], 0.0, W, H)
        loss = F.mse_loss(img.permute(1, 2, 0), target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        first = img.detach() if first is None else first
    return torch.stack(losses), first


# The final-loss gate of the end-to-end test: native / twin after 60 iterations, measured on an MI355X, and the gate at one plus
# twice the observed deviation from 1 (Adam normalises every step, so a coordinate whose gradient is at rounding level moves by
# +-lr in either route; commit 9664932 notes the same effect).
MEASURED_FINAL_RATIO = 0.99999982          # 6.47548295e-04 / 6.47548412e-04
FINAL_RATIO_GATE = 1.0 + 2.0 * abs(1.0 - MEASURED_FINAL_RATIO)


def test_end_to_end_against_the_operator_twin(gpu):
    """60 iterations natively and 60 of the twin.  Measured on an MI355X: final loss native 6.47548295e-04, twin 6.47548412e-04,
    ratio native / twin 0.99999982 (both routes are free of float atomics, so the figure repeats); the gate is one plus twice
    that deviation from 1: 1.00000036."""
    name, iters = "plain", 60
    s = _scene(name)
    sel, _ = _selection(name)
    target = _edit_target(name)
    shs, losses, done = _fit(name, sel).run(target, max_iters=iters, tol=float("-inf"))
    ref, img0 = _twin(name, sel, target, iters)
    assert done == iters and losses.shape == (iters,)
    assert torch.equal(shs[~sel], s["shs"][~sel]), "unselected rows keep their bits"
    assert not torch.equal(shs[sel], s["shs"][sel])
    bound = _loss_bound(img0, target)
    print(f"first loss {float(losses[0]):.8e} twin {float(ref[0]):.8e} bound {bound:.3e}; second {float(losses[1]):.8e} twin {float(ref[1]):.8e}")
    assert abs(float(losses[0]) - float(ref[0])) <= bound
    assert abs(float(losses[1]) - float(ref[1])) <= bound, "the loss after one Adam step"
    assert float(losses[-1]) < float(losses[0])
    ratio = float(losses[-1]) / float(ref[-1])
    print(f"final loss {float(losses[-1]):.8e} twin {float(ref[-1]):.8e} ratio native / twin {ratio:.6f} gate {FINAL_RATIO_GATE}")
    assert FINAL_RATIO_GATE is not None and ratio <= FINAL_RATIO_GATE


def test_dc_rows_only(gpu):
    """sh_rows="dc" with everything selected (optimize_appearance_from_img): rows 1 .. 15 keep their bits, the first two losses
    agree with the twin, the loss falls"""
    name = "clustered"
    s = _scene(name)
    target = _edit_target(name)
    shs, losses, done = _fit(name, None, sh_rows="dc").run(target, max_iters=8, tol=float("-inf"))
    ref, img0 = _twin(name, torch.ones(N, dtype=torch.bool, device="cuda"), target, 2, sh_rows="dc")
    assert done == 8 and torch.equal(shs[:, 1:], s["shs"][:, 1:]) and not torch.equal(shs[:, 0], s["shs"][:, 0])
    bound = _loss_bound(img0, target)
    assert abs(float(losses[0]) - float(ref[0])) <= bound and abs(float(losses[1]) - float(ref[1])) <= bound
    assert float(losses[-1]) < float(losses[0])


def test_early_stop(gpu):
    sel, _ = _selection("plain")
    target = _edit_target("plain")
    shs, losses, done = _fit("plain", sel).run(target, max_iters=50, tol=1e9, check_every=5)
    assert done == 5 and losses.shape == (5,)
    shs, losses, done = _fit("plain", sel).run(target, max_iters=50, tol=1e9, check_every=1)
    assert done == 1 and losses.shape == (1,)
    shs, losses, done = _fit("plain", sel).run(target, max_iters=7, tol=float("-inf"), check_every=5)
    assert done == 7 and losses.shape == (7,)


@pytest.mark.parametrize("masked", (True, False))
def test_fit_appearance(gpu, masked):
    from splatter_a_video_amd.dynamics import FrameClock, frame_preprocess
    from splatter_a_video_amd.tracking import _NAMES
    from splatter_a_video_amd.train_step import synthetic_video_params
    n, w, h, time = 300, 64, 48, 3
    sc = make_scene(n, w, h, F=8, seed=5)
    clock = FrameClock(8)
    params = synthetic_video_params(sc, clock, "cuda", attrs=2)
    extr = _t(sc.extr)

    def render(shs):
        uv, depth, conic, radius, tiles, opa = frame_preprocess(clock, time, extr, w, h, nearest=0.01, extent=1.3,
                                                                **{k: params[k] for k in _NAMES})
        idx, tr = gs.sort_gaussian(uv, depth, w, h, radius, tiles)
        return gs.alpha_blending(uv, conic, opa, OrthoEnhancedRenderer.colors(shs), idx, tr, 0.0, w, h).permute(1, 2, 0).contiguous()

    before = render(params["shs"])
    edited = params["shs"].clone()
    edited[:, 0] += 0.4
    if masked:
        yy, xx = np.mgrid[0:h, 0:w]
        mask = _t(((xx - 30) ** 2 + (yy - 22) ** 2 < 12 ** 2).astype(np.float32))
        target = torch.where(mask[..., None] > 0, render(edited), before)
    else:
        mask, target = None, render(edited)
    keep = {k: v.clone() for k, v in params.items()}
    out, losses = fit_appearance(params, clock, time, extr, w, h, target, mask=mask, max_iters=40, tol=1e-7)
    assert set(out) == set(params)
    for k in params:
        assert torch.equal(params[k], keep[k]), f"the input's {k} was modified"
        assert torch.equal(out[k], params[k]) == (k != "shs"), k
    if not masked:
        assert torch.equal(out["shs"][:, 1:], params["shs"][:, 1:]), "without a mask only the DC row is trained"
    mse0, mse1 = float(F.mse_loss(before, target)), float(F.mse_loss(render(out["shs"]), target))
    print(f"masked={masked}: mse {mse0:.6e} -> {mse1:.6e} after {losses.numel()} iterations")
    assert abs(float(losses[0]) - mse0) <= 1e-4 * mse0 + 1e-9
    assert mse1 < mse0
