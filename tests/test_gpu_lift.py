"""Feature lifting on the GPU (splatter_a_video_amd/lift.py, csrc/lift.hip) against the project's own dense route: with a ones
channel appended to the maps, the autograd gradient of ``(gs.alpha_blending(f) * y * pw).sum()`` with respect to ``f`` [N, D + 1]
IS ``num`` (columns 0 .. D - 1) and ``den`` (column D); and against tests/torch_twin.blend in float64 on one tiny scene.

Bound 1, the project's gradient bound as tests/test_gpu_edit.py applies it: element-wise 2 x (2e-3 |ref| + 1e-4 max |ref|) -- twice the
project's gradient criterion, because both routes carry it against the exact value.

Scenes: the three frozen scenes of tests/test_gpu_edit.py rebuilt here (synth.make_scene seeds 11 / 21 / 31, 1500 Gaussians at
100 x 60, an "opaque" cluster at 0.99, the top right tile emptied): the smallest shapes that still hit partial tiles in both
directions, an empty tile, lists longer than two 64-entry staging batches and pixels that stop well before the end of their list;
``_assert_coverage`` asserts those facts.  The batch tests use a small dynamic model (300 Gaussians, 64 x 48, 8-frame clock)."""
import functools

import numpy as np
import pytest
import torch

from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import gs
from splatter_a_video_amd.lift import FeatureLift, blend_lift, lift_features
from splatter_a_video_amd.synth import make_scene

pytestmark = pytest.mark.gpu

N, W, H = 1500, 100, 60
GX, GY = (W + 15) // 16, (H + 15) // 16
BATCH = 64                       # csrc/lift.hip LIFT_SB
SCENES = ("plain", "opaque", "clustered")
DMAX = 40
WIDTHS = (1, 3, 32, 33, 40)      # a single channel, a few, a full chunk, a chunk tail of 1 and one of 8


def _t(a, dtype=np.float32):
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


@functools.lru_cache(maxsize=None)
def _scene(name):
    """frozen geometry of a seeded scene, sorted once with the pair map (tests/test_gpu_edit.py::_scene)"""
    if name == "plain":
        sc = make_scene(N, W, H, seed=11)
    elif name == "opaque":
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
    return dict(uv=uv, conic=conic, op=_t(op), idx=idx, tr=tr, pm=status.pairmap, culled=_t(reach, bool))


@functools.lru_cache(maxsize=None)
def _maps(name):
    """seeded random maps [DMAX, H, W]; every width of the tests is a leading slice"""
    rng = np.random.default_rng(200 + SCENES.index(name))
    return _t(rng.normal(0.0, 1.0, size=(DMAX, H, W)))


@functools.lru_cache(maxsize=None)
def _pixel_weight():
    pw = torch.ones(H, W, device="cuda")
    pw[7:41, 20:71] = 0.0            # a rectangle that cuts through tiles
    return pw


@functools.lru_cache(maxsize=None)
def _dense(name, weighted=False):
    """the dense route, once per scene: (num [N, DMAX], den [N], ncontrib)"""
    s = _scene(name)
    y = torch.cat([_maps(name), torch.ones(1, H, W, device="cuda")], 0)
    if weighted:
        y = y * _pixel_weight()[None]
    f = torch.zeros(N, DMAX + 1, device="cuda", requires_grad=True)
    img = gs.alpha_blending(s["uv"], s["conic"], s["op"], f, s["idx"], s["tr"], 0.0, W, H)
    (img * y).sum().backward()
    with torch.no_grad():
        _, nc, _ = gs.alpha_blending_enhanced(s["uv"], s["conic"], s["op"], f.detach()[:, :3].contiguous(), s["idx"], s["tr"], 0.0,
                                              W, H, K=1)
    return f.grad[:, :DMAX].contiguous(), f.grad[:, DMAX].contiguous(), nc


def _assert_coverage(name):
    s = _scene(name)
    _, _, nc = _dense(name)
    n = (s["tr"][:, 1] - s["tr"][:, 0]).cpu().numpy().reshape(GY, GX)
    assert W % 16 and H % 16, "partial tiles in both directions"
    assert n[0, GX - 1] == 0 and (n == 0).sum() >= 1, "an empty tile"
    assert n.max() > 2 * BATCH, f"a list longer than two staging batches: longest {n.max()}"
    per_pixel = np.repeat(np.repeat(n, 16, 0), 16, 1)[:H, :W]
    last = nc.cpu().numpy()
    assert (last <= per_pixel).all()
    assert ((last < per_pixel) & (last > 0)).sum() >= 100, "pixels whose last contributor lies below their list length"
    if name == "opaque":     # pixels that stopped: saturated well before the end of a long list
        assert (last < per_pixel // 2).sum() >= 20
    print(f"{name}: lists up to {n.max()}, {(n == 0).sum()} empty tiles, last < n on {(last < per_pixel).sum()} pixels")


def _assert_close(got, ref, what):
    """bound 1"""
    a, b = got.double().cpu().numpy(), ref.double().cpu().numpy()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all(), f"{what}: not finite"
    assert np.abs(b).max() > 0
    lim = 2.0 * (2e-3 * np.abs(b) + 1e-4 * np.abs(b).max())
    err = np.abs(a - b)
    print(f"{what}: max |ref| {np.abs(b).max():.3e}, worst err / bound {float((err / lim).max()):.4f}")
    assert (err <= lim).all(), f"{what}: {int((err > lim).sum())} of {err.size} off, worst {float((err / lim).max()):.2f} x the bound"


def _lift(name, maps, pw=None):
    s = _scene(name)
    return blend_lift(s["uv"], s["conic"], s["op"], s["idx"], s["tr"], s["pm"], maps, W, H, pw)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("name", SCENES)
def test_kernel_against_the_dense_route(gpu, name, D):
    _assert_coverage(name)
    num_ref, den_ref, _ = _dense(name)
    num, den = _lift(name, _maps(name)[:D].contiguous())
    assert num.shape == (N, D) and den.shape == (N,)
    _assert_close(num, num_ref[:, :D], f"{name} D={D} num")
    _assert_close(den, den_ref, f"{name} D={D} den")
    culled = _scene(name)["culled"]
    assert int(culled.sum()) > 0 and (den[culled] == 0).all() and (num[culled] == 0).all()


def test_against_float64(gpu):
    """one tiny scene (40 Gaussians, 40 x 24) against tests/torch_twin.blend in float64 on the CPU, in the same way: the check is
    not GPU against GPU only"""
    import torch_twin
    n, w, h, D = 40, 40, 24, 3
    sc = make_scene(n, w, h, seed=3, sigma_px=3.0)
    uv, depth, conic, radius, tiles = gs.preprocess_ortho(_t(sc.xyz), _t(sc.scale), _t(sc.rotate), _t(sc.extr), w, h, nearest=0.01)
    op = _t(sc.opacity)
    idx, tr, status = gs.sort_gaussian_capped(uv, depth, w, h, radius, None)
    rng = np.random.default_rng(9)
    maps = rng.normal(size=(D, h, w)).astype(np.float32)
    pw = rng.uniform(0.5, 1.5, size=(h, w)).astype(np.float32)
    pw[5:13, 11:30] = 0.0
    num, den = blend_lift(uv, conic, op, idx, tr, status.pairmap, _t(maps), w, h, _t(pw))
    f = torch.zeros(n, D + 1, dtype=torch.float64, requires_grad=True)
    out, _, nc, _ = torch_twin.blend(uv.cpu().double(), conic.cpu().double(), op.cpu().double(), f, idx.cpu(), tr.cpu(), 0.0, w, h)
    assert int(nc.max()) >= 3, "pixels with several contributors"
    y = torch.cat([torch.tensor(maps, dtype=torch.float64), torch.ones(1, h, w, dtype=torch.float64)], 0)
    (out * y * torch.tensor(pw, dtype=torch.float64)[None]).sum().backward()
    _assert_close(num, f.grad[:, :D], "float64 num")
    _assert_close(den, f.grad[:, D], "float64 den")


@pytest.mark.parametrize("name", ("plain", "opaque"))
def test_pixel_weight(gpu, name):
    """zeros over a rectangle that cuts through tiles, NaN written into the maps inside it: the result is finite and equals the
    dense route on the weighted, NaN-free maps"""
    D = 33
    num_ref, den_ref, _ = _dense(name, True)
    maps = _maps(name)[:D].clone()
    maps[:, 7:41, 20:71] = float("nan")
    num, den = _lift(name, maps, _pixel_weight())
    assert torch.isfinite(num).all() and torch.isfinite(den).all()
    _assert_close(num, num_ref[:, :D], f"{name} weighted num")
    _assert_close(den, den_ref, f"{name} weighted den")
    # a Gaussian seen only under the rectangle gets exactly zero
    zero = den_ref == 0
    assert int(zero.sum()) > int(_scene(name)["culled"].sum())
    assert (den[zero] == 0).all() and (num[zero] == 0).all()


@pytest.mark.parametrize("name", SCENES)
def test_constant_map(gpu, name):
    """y = c: num / den = c within n 2^-24 relative, n = the number of (pixel, frame) terms of the Gaussian's sums, bounded by
    256 x tiles touched x F (both sums add n non-negative multiples of the same weights; a sum of n non-negative float32 terms
    carries at most n 2^-24 relative)"""
    s = _scene(name)
    c = torch.tensor([0.7, -3.25, 1e-3], device="cuda")
    num, den = _lift(name, c[:, None, None].expand(3, H, W).contiguous())
    goff = s["pm"].goff.long()
    touched = torch.diff(goff, prepend=goff.new_zeros(1))
    seen = den > 0
    assert int(seen.sum()) > 0 and int((~seen).sum()) > 0, "Gaussians of both kinds"
    assert (touched[seen] > 0).all()
    feature = num[seen].double() / den[seen].double()[:, None]
    rel = ((feature - c.double()) / c.double()).abs()
    bound = (256.0 * touched[seen].double() * 2.0 ** -24)[:, None]
    print(f"{name}: worst relative deviation {float(rel.max()):.3e}, worst / bound {float((rel / bound).max()):.4f}")
    assert (rel <= bound).all()
    assert (num[~seen] == 0).all()


# ------------------------------------------------------------------ a small dynamic model: batches of frames
DN, DW, DH, CLIP = 300, 64, 48, 8
TIMES = (1, 3, 6)
HIDDEN = 7                       # Gaussians moved out of view: unseen in every frame


@functools.lru_cache(maxsize=None)
def _model():
    from splatter_a_video_amd.dynamics import FrameClock
    from splatter_a_video_amd.tracking import _NAMES
    from splatter_a_video_amd.train_step import synthetic_video_params
    sc = make_scene(DN, DW, DH, F=CLIP, seed=5)
    clock = FrameClock(CLIP)
    params = synthetic_video_params(sc, clock, "cuda", attrs=2, cubic_sigma=0.02)
    params = {k: params[k] for k in _NAMES}
    params["position"][:HIDDEN, 0] = 5.0
    return params, clock, _t(sc.extr)


@functools.lru_cache(maxsize=None)
def _frame_lists(time):
    """one frame's geometry and sorted lists through the single-frame operators"""
    from splatter_a_video_amd.dynamics import frame_preprocess
    params, clock, extr = _model()
    with torch.no_grad():
        uv, depth, conic, radius, tiles, opa = frame_preprocess(clock, time, extr, DW, DH, nearest=0.01, extent=1.3, **params)
    idx, tr, status = gs.sort_gaussian_capped(uv, depth, DW, DH, radius, None, conic, opa)
    return uv, conic, opa, idx, tr, status.pairmap


@functools.lru_cache(maxsize=None)
def _clip_maps(D):
    rng = np.random.default_rng(77 + D)
    return _t(rng.normal(size=(len(TIMES), D, DH, DW)))


def _feature_lift(D, **kw):
    params, clock, extr = _model()
    return FeatureLift(params, clock, extr, DW, DH, D, **kw)


def test_batch(gpu):
    """FeatureLift.add over three frames of distinct geometry = the sum of three single-frame blend_lift calls: within bound 1 on
    the lists of dynamics.frame_preprocess + gs.sort_gaussian_capped (same uv, opacity, lists and pair map, bit for bit, but the
    batched preprocess rounds a conic differently in the last place -- measured: up to 3e-7 absolute -- so the weights differ at
    rounding level), and bit for bit on the batch's own geometry rows: the fold adds each frame's own sum, slots ascending, onto
    the running value, frames ascending.  Adds split 2 + 1, and batches of two frames (a padded last batch), give the same bits."""
    D = 35
    maps = _clip_maps(D)
    geo = [_frame_lists(t) for t in TIMES]
    assert not torch.equal(geo[0][0], geo[1][0]) and not torch.equal(geo[1][0], geo[2][0]), "the geometry differs per frame"
    parts = [blend_lift(*g, maps[i], DW, DH) for i, g in enumerate(geo)]
    one = _feature_lift(D, frames_per_batch=4).add(TIMES, maps)
    _assert_close(one.num, (parts[0][0] + parts[1][0]) + parts[2][0], "batch num")
    _assert_close(one.den, (parts[0][1] + parts[1][1]) + parts[2][1], "batch den")
    fb, own = one.fb, []
    for i, (uv, conic, opa, idx, tr, pm) in enumerate(geo):
        M = idx.numel()
        assert torch.equal(fb.uv[i], uv) and torch.equal(one.opa_t, opa) and torch.equal(fb.tile_range[i], tr)
        assert int(fb.pairs[i]) == M and torch.equal(fb.idx_sorted[i, :M], idx) and torch.equal(fb.goff[i], pm.goff)
        assert torch.equal(fb.slot_sorted[i, :M], pm.slot_sorted)
        own.append(blend_lift(uv, fb.conic[i], opa, idx, tr, pm, maps[i], DW, DH))
    num_ref, den_ref = (own[0][0] + own[1][0]) + own[2][0], (own[0][1] + own[1][1]) + own[2][1]
    assert torch.equal(one.num, num_ref) and torch.equal(one.den, den_ref), "(frame, slot) ascending: bit for bit"
    split = _feature_lift(D, frames_per_batch=4).add(TIMES[:2], maps[:2]).add(TIMES[2:], maps[2:])
    assert torch.equal(split.num, one.num) and torch.equal(split.den, one.den)
    two = _feature_lift(D, frames_per_batch=2).add(TIMES, maps)
    assert torch.equal(two.num, one.num) and torch.equal(two.den, one.den)
    feature, weight = one.result()
    assert torch.equal(weight, one.den) and torch.isfinite(feature).all()
    assert (weight[:HIDDEN] == 0).all() and (feature[:HIDDEN] == 0).all(), "an unseen Gaussian gets 0, never NaN"
    assert (weight[HIDDEN:] > 0).sum() > DN // 2
    f2, w2 = lift_features(*_model()[:2], TIMES, _model()[2], DW, DH, maps, frames_per_batch=4)
    assert torch.equal(f2, feature) and torch.equal(w2, weight)


def test_constant_map_over_a_clip(gpu):
    params, clock, extr = _model()
    c = 2.5
    maps = torch.full((len(TIMES), 1, DH, DW), c, device="cuda")
    feature, weight = lift_features(params, clock, TIMES, extr, DW, DH, maps)
    seen = weight > 0
    assert int(seen.sum()) > 0 and int((~seen).sum()) >= HIDDEN
    tiles = ((DW + 15) // 16) * ((DH + 15) // 16)            # (an upper bound of the tiles a Gaussian touches)
    rel = ((feature[seen, 0].double() - c) / c).abs()
    assert float(rel.max()) <= 256.0 * tiles * len(TIMES) * 2.0 ** -24
    assert (feature[~seen] == 0).all()


def test_reproducibility(gpu):
    D = 33
    maps = _clip_maps(D)
    pw = torch.ones(len(TIMES), DH, DW, device="cuda")
    pw[:, 10:30, 5:40] = 0.25
    runs = [_feature_lift(D, frames_per_batch=2).add(TIMES, maps, pw) for _ in range(2)]
    old = L.deterministic()
    try:
        L.set_deterministic(True)
        runs += [_feature_lift(D, frames_per_batch=2).add(TIMES, maps, pw) for _ in range(2)]
    finally:
        L.set_deterministic(old)
    assert L.deterministic() == old
    assert float(runs[0].num.abs().max()) > 0
    for r in runs[1:]:
        assert torch.equal(r.num, runs[0].num) and torch.equal(r.den, runs[0].den)


def test_capacity(gpu):
    """a batch that outgrows its pair capacity is binned again with a larger one, never folded in partially"""
    D = 4
    maps = _clip_maps(D)
    roomy = _feature_lift(D, frames_per_batch=2).add(TIMES, maps)
    small = _feature_lift(D, frames_per_batch=2, capacity=64)
    assert max(g[3].numel() for g in (_frame_lists(t) for t in TIMES)) > 64
    small.add(TIMES, maps)
    assert small.regrows >= 1 and roomy.regrows == 0
    assert torch.equal(small.num, roomy.num) and torch.equal(small.den, roomy.den)


def _dense_loss(feature, maps):
    """1/2 sum (A f - y)^2 over the clip through the single-frame operators, differentiable in feature"""
    loss = 0.0
    for i, t in enumerate(TIMES):
        uv, conic, opa, idx, tr, _ = _frame_lists(t)
        img = gs.alpha_blending(uv, conic, opa, feature, idx, tr, 0.0, DW, DH)
        loss = loss + 0.5 * ((img - maps[i]) ** 2).sum()
    return loss


def test_refine(gpu):
    D = 5
    gen = torch.Generator(device="cuda").manual_seed(13)
    f_star = torch.rand(DN, D, device="cuda", generator=gen) * 2.0 - 1.0
    with torch.no_grad():
        maps = torch.stack([gs.alpha_blending(*_frame_lists(t)[:3], f_star, *_frame_lists(t)[3:5], 0.0, DW, DH) for t in TIMES])
    lift = _feature_lift(D, frames_per_batch=2).add(TIMES, maps)
    start, _ = lift.result()
    # one iteration's gradient against the dense autograd gradient of the same loss
    f = start.clone().requires_grad_(True)
    loss_ref = _dense_loss(f, maps)
    loss_ref.backward()
    grad, loss = lift.gradient(TIMES, maps, start)
    _assert_close(grad, f.grad, "refine gradient")
    assert abs(float(loss) - float(loss_ref.detach())) <= 1e-3 * float(loss_ref.detach())
    iters = 50
    fitted, history = lift.refine(TIMES, maps, start, iters, lr=0.01)
    assert history.is_cuda and history.shape == (iters,) and fitted.shape == (DN, D)
    assert torch.equal(history[:1], loss), "the first entry is the loss at the lifted start"
    final = float(lift.gradient(TIMES, maps, fitted)[1])
    print(f"loss at the lifted start {float(history[0]):.6e}, after {iters} iterations {final:.6e}")
    assert final < float(history[0])
    assert not torch.equal(fitted, start) and torch.equal(start, lift.result()[0]), "the start is not modified"
    # forward-only with respect to the model
    params, clock, extr = _model()
    live = dict(params)
    live["position"] = params["position"].clone().requires_grad_(True)
    with pytest.raises(ValueError, match="forward-only"):
        FeatureLift(live, clock, extr, DW, DH, D).refine(TIMES, maps, start, 2)
