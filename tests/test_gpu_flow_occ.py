"""Where a dense flow is valid, on the GPU (splatter_a_video_amd.flow; csrc/flow.hip; include/splat_hip_flow_occ.h): the flow
attribute with the depth and its gradient against the float64 restatement of tests/flow_occ_ref.py, the fused occlusion kernel
against its float32 restatement (bits), ``render_flow(scene_flow=True)`` against the frame batch fed with the attribute (bits),
and ``render_flow(occlusion=True, cycle=True)`` on a scene with a known occluder, its regions read off depth renders."""
import itertools

import numpy as np
import pytest
import torch

import flow_occ_ref as OR
import flow_ref as FR
from test_gpu_flow import FRAMES, P, PAIRS, T_CLIP, _attr_call, _cameras, _direct_backward, _grad_close, _hand_placed
from test_gpu_layers import H, N, NAMES, W, Scene, _dynamic_host, _t

pytestmark = pytest.mark.gpu

KINDS = ["ortho", "ortho_per_pair", "pinhole", "extr2", "pinhole_extr2"]


@pytest.fixture(scope="module")
def model(gpu):
    clock, host, _ = _dynamic_host(P, FRAMES, 11)
    return clock, host


def _ref4(clock, host, t1, t2, cams, zero=False, g=None, position=None, cubic=None):
    e, i_, e2, i2, nearest = cams
    return OR.attribute4(clock, t1, t2, host["position"] if position is None else position,
                         host["pos_cubic_node"] if cubic is None else cubic, e, i_, e2, i2, W, H, nearest, 1.3, zero, g=g)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. attribute with the depth, forward
@pytest.mark.parametrize("F", [1, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_attribute_depth_forward_against_float64(model, kind, F):
    clock, host = model
    t1, t2 = PAIRS[F]
    cams = _cameras(kind, F)
    ref = _ref4(clock, host, t1, t2, cams)
    got_t = _attr_call(clock, host, t1, t2, cams, depth=True)
    assert got_t.shape == (F, P, 4)
    two = _attr_call(clock, host, t1, t2, cams)
    assert torch.equal(_bits(got_t[..., :2]), _bits(two))                   # channels 0, 1: the two-channel entry point's bits
    seg = _attr_call(clock, host, t1, t2, cams, layout=1, depth=True)
    assert torch.equal(_bits(seg), _bits(got_t))                            # both layouts: the same arithmetic
    got = got_t.cpu().numpy().astype(np.float64)
    keep = ~ref["near"]
    err = np.abs(got - ref["attr"])[..., 2:]
    bound = ref["bound"][..., 2:]
    live = bound > 0
    ratio = (err / np.where(live, bound, 1.0))[keep]
    print(f"{kind} F={F}: left out {1 - keep.mean():.3%}, depth channels max err / bound {float(ratio.max()):.3f}, "
          f"max bound {bound.max():.3e}, max |dz| {np.abs(ref['attr'][..., 2]).max():.3f}, culled at t2 {ref['cull2'].mean():.3%}")
    assert 1 - keep.mean() <= 0.01
    assert (err <= bound)[keep].all()                                        # a culled side: bound 0, an exact 0
    assert bound.max() < 15 * OR.EPS * 16 and np.abs(ref["attr"][..., 2]).max() > 1e-3      # |z| terms of a few units; it moves in depth
    # a side culled at t2 has z2 = 0 exactly
    c2 = ref["cull2"] & keep
    assert (got_t[..., 3].cpu().numpy()[c2].view(np.int32) == 0).all()


@pytest.mark.parametrize("kind", ["ortho_per_pair", "pinhole"])
def test_identical_pairs_are_plus_zero_in_three_channels(model, kind):
    clock, host = model
    t1, _ = PAIRS[7]
    for layout in (0, 1):
        out = _attr_call(clock, host, t1, t1, _cameras(kind, 7), layout=layout, depth=True)
        assert int(_bits(out[..., :3]).count_nonzero()) == 0
        assert float(out[..., 3].abs().max()) > 1.0                          # z2 itself is there


@pytest.mark.parametrize("kind", ["ortho", "pinhole_extr2"])
def test_hand_placed_cull_decisions_with_depth(gpu, kind):
    from splatter_a_video_amd.dynamics import FrameClock
    clock = FrameClock(FRAMES)
    pos, cub = _hand_placed(clock)
    e, i_, e2, i2, _ = _cameras(kind, 1)
    e = np.eye(4, dtype=np.float32)
    cams = (e, i_, None if e2 is None else e, i2, 0.3)
    for zero in (False, True):
        ref = _ref4(clock, None, [0.0], [29.0], cams, zero=zero, position=pos, cubic=cub)
        assert ref["cull1"][0].tolist() == [True, False, True, True, True] and ref["cull2"][0].tolist() == [False, True, True, False, True]
        assert not ref["near"].any()
        got = _attr_call(clock, None, [0.0], [29.0], cams, zero=zero, position=_t(pos), cubic=_t(cub), depth=True).cpu().numpy()[0]
        for n in range(5):
            c1, c2 = ref["cull1"][0, n], ref["cull2"][0, n]
            if (c1 and c2) or (zero and (c1 or c2)):
                assert got[n].view(np.int32).tolist() == [0, 0, 0, 0], (kind, zero, n)       # four +0.0
            elif c2:                                                                       # z2 = 0 exactly: (-uv1, -z1, 0)
                assert got[n, 3:].view(np.int32).tolist() == [0] and np.isclose(got[n, 2], -ref["z1"][0, n], rtol=1e-5), (kind, zero, n)
            else:                                                                          # c1: z1 = 0 exactly: (uv2, z2, z2)
                assert got[n, 2] == got[n, 3] and np.isclose(got[n, 3], ref["z2"][0, n], rtol=1e-5) and got[n, 3] > 0.3, (kind, zero, n)


# ------------------------------------------------------------------ 2. attribute with the depth, backward
@pytest.mark.parametrize("kind", KINDS)
def test_attribute_depth_backward_against_float64(model, kind):
    from splatter_a_video_amd import _lib as L
    clock, host = model
    t1, t2 = PAIRS[7]
    cams = _cameras(kind, 7)
    rng = np.random.default_rng(3)
    g = rng.normal(size=(7, P, 4)).astype(np.float32)
    ref = _ref4(clock, host, t1, t2, cams, g=g)
    pos, cub = _t(host["position"]), _t(host["pos_cubic_node"])
    d_pos, d_cub = _direct_backward(clock, (pos, cub), t1, t2, cams, _t(g))
    _grad_close(d_pos.cpu().numpy(), ref["d_position"], f"{kind} d_position")
    _grad_close(d_cub.cpu().numpy(), ref["d_cubic"], f"{kind} d_pos_cubic_node")
    # the depth gradient is there: without it the result differs
    uv_only = _direct_backward(clock, (pos, cub), t1, t2, cams, _t(g[..., :2]))
    assert not torch.equal(uv_only[0], d_pos)
    # g[..., 2:] = 0: the bits of the two-channel backward
    g0 = g.copy()
    g0[..., 2:] = 0.0
    zeroed = _direct_backward(clock, (pos, cub), t1, t2, cams, _t(g0))
    assert torch.equal(_bits(zeroed[0]), _bits(uv_only[0])) and torch.equal(_bits(zeroed[1]), _bits(uv_only[1]))
    # two runs, the second in deterministic mode: the same bits
    L.set_deterministic(True)
    try:
        again = _direct_backward(clock, (pos, cub), t1, t2, cams, _t(g))
    finally:
        L.set_deterministic(False)
    assert torch.equal(again[0], d_pos) and torch.equal(again[1], d_cub)
    # autograd through flow_attribute(depth=True) is the direct call
    pa, ca = pos.clone().requires_grad_(True), cub.clone().requires_grad_(True)
    _attr_call(clock, host, t1, t2, cams, position=pa, cubic=ca, depth=True).backward(_t(g))
    assert torch.equal(pa.grad, d_pos) and torch.equal(ca.grad, d_cub)


@pytest.mark.parametrize("zero", [False, True])
def test_depth_backward_culled_sides_get_exactly_zero(gpu, zero):
    from splatter_a_video_amd.dynamics import FrameClock
    clock = FrameClock(FRAMES)
    I = clock.interval_num
    pos, cub = _hand_placed(clock)
    cams = (np.eye(4, dtype=np.float32), None, None, None, 0.3)
    g = np.array([[[1.5, -2.0, 0.75, -1.25]] * 5], np.float32)
    ref = _ref4(clock, None, [0.0], [29.0], cams, zero=zero, g=g, position=pos, cubic=cub)
    d_pos, d_cub = _direct_backward(clock, (_t(pos), _t(cub)), [0.0], [29.0], cams, _t(g), zero=zero)
    d_pos, d_cub = d_pos.cpu().numpy(), d_cub.cpu().numpy().reshape(5, 4, I, 3)
    _grad_close(d_pos, ref["d_position"], "hand-placed d_position")
    _grad_close(d_cub, ref["d_cubic"], "hand-placed d_pos_cubic_node")
    assert (d_cub[:, :, 1:I - 1] == 0).all()
    for n, (c1, c2) in enumerate(zip(ref["cull1"][0], ref["cull2"][0])):
        dead1, dead2 = c1 or (zero and c2), c2 or (zero and c1)
        assert (d_cub[n, :, 0] == 0).all() == bool(dead1), n
        assert (d_cub[n, :, I - 1] == 0).all() == bool(dead2), n
        if dead1 and dead2:
            assert (d_pos[n] == 0).all(), n
        if not dead2:
            assert d_cub[n, 3, I - 1, 2] == np.float32(0.75) + np.float32(-1.25)             # identity camera: g.z + g.w on side 2


# ------------------------------------------------------------------ 3. the fused kernel on synthetic maps
PARAMS = dict(bg_depth=1.0, depth_margin=0.05, min_coverage=0.5, fb_alpha=0.01, fb_beta=0.5)


def _synthetic(Hs, Ws, F=3, seed=0):
    """random planes, flows up to +-12 px; planted: integer flows, q exactly on W - 1 / H - 1, targets outside on every side,
    NaN and inf components, coverage on both sides of min_coverage and exactly at it"""
    rng = np.random.default_rng(seed)
    flow = np.clip(rng.normal(0, 4.0, size=(F, 2, Hs, Ws)), -12, 12).astype(np.float32)
    for c, n in ((0, Ws), (1, Hs)):                     # a thin map: most pixels stay inside along the thin axis
        if n < 8:
            flow[:, c][rng.uniform(size=(F, Hs, Ws)) < 0.7] = 0.0
    ys, xs = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    pick = lambda p: rng.uniform(size=(Hs, Ws)) < p
    for f in range(F):
        m = pick(0.15)
        flow[f, :, m] = np.round(flow[f, :, m])                              # integer flows: fx = fy = 0
        m = pick(0.04)
        flow[f, 0][m] = (Ws - 1 - xs)[m]                                     # q exactly on W - 1
        m = pick(0.04)
        flow[f, 1][m] = (Hs - 1 - ys)[m]                                     # ... on H - 1
        for c, tgt in ((0, -xs - 0.25), (0, Ws - xs - 0.5), (1, -ys - 1.0), (1, Hs - ys + 0.0), (0, -xs - 2.0 ** -20)):
            m = pick(0.02)
            flow[f, c][m] = tgt[m].astype(np.float32)                        # outside on every side, one barely
        for c, val in ((0, np.nan), (1, np.nan), (0, np.inf), (1, -np.inf)):
            flow[f, c][pick(0.01)] = val
    cov = rng.uniform(0, 1, size=(F, Hs, Ws)).astype(np.float32)
    cov[rng.uniform(size=cov.shape) < 0.1] = 0.5                             # exactly at min_coverage: covered
    cov[rng.uniform(size=cov.shape) < 0.05] = np.nextafter(np.float32(0.5), np.float32(0))
    cov[rng.uniform(size=cov.shape) < 0.3] = 1.0
    track = rng.uniform(2.0, 4.0, size=(F, Hs, Ws)).astype(np.float32)
    surface = (track + rng.normal(0, 0.1, size=track.shape)).astype(np.float32)
    back = (-flow + rng.normal(0, 0.5, size=flow.shape)).astype(np.float32)
    back[~np.isfinite(back)] = 1.0
    src = rng.normal(0, 1.0, size=(F, 8, Hs, Ws)).astype(np.float32)
    return dict(flow=flow, coverage=cov, track_depth=track, surface=surface, flow_back=back, src=src)


def _same_bits(got, want, name):
    assert (got is None) == (want is None), name
    if want is not None:
        got = got.cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype, name
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"{name}: {int((got.view(np.int32) != want.view(np.int32)).sum())} differ"


@pytest.mark.parametrize("size", [(45, 53), (1, 53), (45, 1), (44, 52)])      # the last: H W a multiple of 4, the kernel's wide runs
def test_fused_kernel_is_its_float32_restatement(gpu, size):
    from splatter_a_video_amd.flow import flow_occlusion
    Hs, Ws = size
    d = _synthetic(Hs, Ws, seed=Hs * 100 + Ws)
    dev = {k: _t(v) for k, v in d.items()}
    seen = np.zeros(4, np.int64)
    for depth, cov, back, C in itertools.product((False, True), (False, True), (False, True), (0, 1, 3, 8)):
        kw = dict(track_depth=d["track_depth"] if depth else None, surface=d["surface"] if depth else None,
                  coverage=d["coverage"] if cov else None, flow_back=d["flow_back"] if back else None,
                  src=d["src"][:, :C] if C else None)
        want = OR.occlusion(d["flow"], **kw, **PARAMS)
        pick = lambda k, on: dev[k] if on else None
        got = flow_occlusion(dev["flow"], track_depth=pick("track_depth", depth), surface_depth=pick("surface", depth),
                             coverage=pick("coverage", cov), flow_back=pick("flow_back", back),
                             src=dev["src"][:, :C] if C else None, counts=True, **PARAMS)
        name = f"{size} depth={depth} coverage={cov} back={back} C={C}"
        assert got.mask.dtype == torch.uint8 and np.array_equal(got.mask.cpu().numpy(), want["mask"]), name
        assert got.counts.cpu().numpy().tolist() == want["counts"].tolist(), name
        _same_bits(got.depth_gap, want["depth_gap"], name + " depth_gap")
        _same_bits(got.fb_sq, want["fb_sq"], name + " fb_sq")
        _same_bits(got.warped, want["warped"], name + " warped")
        if depth and cov and back:
            seen = want["counts"].sum(0)
            assert flow_occlusion(dev["flow"], coverage=dev["coverage"], **PARAMS).counts is None      # not asked: none
    print(f"{size}: pixels per bit {seen.tolist()} of {3 * Hs * Ws}")
    assert (seen > 0).all()                                                  # every decision occurs, both ways
    assert (seen < 3 * Hs * Ws).all()


def test_planted_pixels_take_the_planted_decisions(gpu):
    """the float64 twin agrees with the kernel wherever its own decision is clear, and the planted edge cases are where they
    were planted: q on W - 1 is inside, 2^-20 beyond 0 is outside, coverage exactly at min_coverage is covered"""
    from splatter_a_video_amd.flow import OUTSIDE, UNCOVERED, flow_occlusion
    Hs, Ws = 45, 53
    d = _synthetic(Hs, Ws, seed=7)
    got = flow_occlusion(_t(d["flow"]), coverage=_t(d["coverage"]), **PARAMS).mask.cpu().numpy()
    ys, xs = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    u, v = d["flow"][:, 0], d["flow"][:, 1]
    fin = np.isfinite(u) & np.isfinite(v)
    on_edge = fin & (u == (Ws - 1 - xs)) & (ys + v >= 0) & (ys + v <= Hs - 1)
    assert on_edge.sum() > 50 and not (got[on_edge] & OUTSIDE).any()
    barely = fin & (u == (-xs - 2.0 ** -20).astype(np.float32)) & (xs < 16)             # x + u = -2^-20 survives float32 for small x
    assert barely.sum() > 5 and (got[barely] & OUTSIDE).all()
    assert (got[~fin] & OUTSIDE).all() and (~fin).sum() > 50
    assert not (got[d["coverage"] == 0.5] & UNCOVERED).any() and (got[d["coverage"] < 0.5] & UNCOVERED).all()


def test_warp_by_a_zero_flow_is_the_source(gpu):
    from splatter_a_video_amd.flow import warp_by_flow
    rng = np.random.default_rng(2)
    for Hs, Ws in ((45, 53), (44, 52)):
        src = _t(rng.normal(size=(2, 3, Hs, Ws)))
        warped, valid = warp_by_flow(src, torch.zeros(2, 2, Hs, Ws, device="cuda"))
        assert torch.equal(_bits(warped), _bits(src)) and valid.dtype == torch.bool and bool(valid.all())
        shift = torch.zeros(2, 2, Hs, Ws, device="cuda")
        shift[:, 0] = 1.0                                                    # one pixel to the right: the last column leaves
        warped, valid = warp_by_flow(src, shift)
        assert torch.equal(warped[..., :-1], src[..., 1:]) and not bool(valid[..., -1].any()) and bool(valid[..., :-1].all())
        assert int(_bits(warped[..., -1]).count_nonzero()) == 0


# ------------------------------------------------------------------ 4. render_flow(scene_flow=True)
@pytest.fixture(scope="module")
def scene(gpu):
    sc = Scene()
    sc.geo = {k: sc.model[k] for k in NAMES}
    return sc


def _render(sc, **kw):
    from splatter_a_video_amd.flow import render_flow
    with torch.no_grad():
        return render_flow(dict(sc.model), sc.clock, T_CLIP[0], T_CLIP[1], sc.extr, W, H, frames_per_batch=2, cubic_layout=0, **kw)


def test_scene_flow_is_the_frame_batch_fed_with_the_attribute(scene):
    from splatter_a_video_amd.flow import flow_attribute
    from splatter_a_video_amd.frames import FrameBatch
    sc = scene
    out = _render(sc, scene_flow=True, coverage=True)
    assert sorted(out) == ["coverage", "flow", "scene_flow", "track_depth"]
    assert out["flow"].shape == (5, 2, H, W) and all(out[k].shape == (5, 1, H, W) for k in ("coverage", "scene_flow", "track_depth"))
    fb = FrameBatch(2, N, W, H, 5, "cuda", records=False)
    ones = torch.ones(N, 1, device="cuda")
    pad = [0, 1, 2, 3, 4, 4]
    with torch.no_grad():
        for b0 in (0, 2, 4):
            t1, t2 = [T_CLIP[0][i] for i in pad[b0:b0 + 2]], [T_CLIP[1][i] for i in pad[b0:b0 + 2]]
            attr = flow_attribute(sc.clock, t1, t2, sc.extr, W, H, position=sc.geo["position"], pos_cubic_node=sc.geo["pos_cubic_node"],
                                  depth=True)
            row = fb.render_dynamic_sets(sc.clock, t1, sc.extr, [dict(feature=[attr, ones], bg=0.0, detach_opacity=True)],
                                         cubic_layout=0, **sc.geo)[0]
            fb.check()
            n = min(2, 5 - b0)
            for k, c0, c1 in (("flow", 0, 2), ("scene_flow", 2, 3), ("track_depth", 3, 4), ("coverage", 4, 5)):
                assert torch.equal(out[k][b0:b0 + n], row[:n, c0:c1]), k
    assert float(out["scene_flow"].abs().max()) > 1e-3 and 1.5 < float(out["track_depth"].max()) < 4.5
    # no new keys without the flags, and the flow is the default call's within the image rule
    plain = _render(sc)
    assert sorted(plain) == ["flow"] and sorted(_render(sc, coverage=True)) == ["coverage", "flow"]
    err = float((plain["flow"] - out["flow"]).abs().max())
    print(f"flow of the scene-flow row against the default call: max err {err:.3e}")
    assert torch.allclose(out["flow"], plain["flow"], rtol=1e-4, atol=1e-5)


def test_scene_flow_differentiable_and_occlusion_forward_only(scene):
    from splatter_a_video_amd.flow import render_flow
    sc = scene
    live = lambda: dict(sc.model, position=sc.model["position"].clone().requires_grad_(True),
                        pos_cubic_node=sc.model["pos_cubic_node"].clone().requires_grad_(True))
    call = lambda m, **kw: render_flow(m, sc.clock, T_CLIP[0], T_CLIP[1], sc.extr, W, H, frames_per_batch=2, cubic_layout=0, **kw)
    with pytest.raises(ValueError, match="not differentiable"):
        call(live(), occlusion=True, differentiable=True)
    with pytest.raises(ValueError, match="cycle=True needs occlusion=True"):
        call(live(), cycle=True)
    grads = []
    for _ in range(2):
        m = live()
        out = call(m, scene_flow=True, differentiable=True)
        assert out["track_depth"].requires_grad and out["scene_flow"].requires_grad
        out["track_depth"].sum().backward()
        grads.append((m["position"].grad, m["pos_cubic_node"].grad))
    for g in grads[0]:
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert float(grads[0][0][:, 2].abs().max()) > 0                          # the depth pulls on z
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    with torch.no_grad():
        assert torch.equal(out["track_depth"].detach(), _render(sc, scene_flow=True)["track_depth"])


# ------------------------------------------------------------------ 5. a scene with a known occluder
SHIFT_PX = 4.5          # the cluster's displacement: a pixel of region C is covered by the cluster to > 90 % (depth1 < 2.1), its
#                         flow is that share of the displacement: within 0.45 px of it
MARGIN_PX = 6


class Occluder:
    """a dense static layer of opaque Gaussians at depth 3 over the whole frame, and a compact opaque cluster at depth 2, a tall
    block, that sits left at time 0 and SHIFT_PX further right at time 29: constant coefficients per segment (the block does
    not move inside a segment).  The depths are spread by +-0.01 so that no two Gaussians tie in the sort."""

    def __init__(self):
        from splatter_a_video_amd.dynamics import FrameClock
        self.clock = FrameClock(FRAMES)
        I = self.clock.interval_num
        rng = np.random.default_rng(9)
        px = 2.0 / W                                                          # a pixel in world units, both axes (ortho: [-1, 1])
        py = 2.0 / H
        gx, gy = np.meshgrid(np.arange(-3, W + 3, 1.5), np.arange(-3, H + 3, 1.5))
        layer = np.stack([(gx.ravel() + 0.5) * px - 1.0, (gy.ravel() + 0.5) * py - 1.0, np.full(gx.size, 3.0)], 1)
        cx, cy = np.meshgrid(np.arange(30, 44, 1.0), np.arange(5, 59, 1.0))   # 14 x 54 px at time 0
        block = np.stack([(cx.ravel() + 0.5) * px - 1.0, (cy.ravel() + 0.5) * py - 1.0, np.full(cx.size, 2.0)], 1)
        pos = np.concatenate([layer, block]).astype(np.float32)
        n = pos.shape[0]
        pos[:, 2] += rng.permutation(n).astype(np.float32) / n * 0.02 - 0.01
        self.n, self.n_layer = n, layer.shape[0]
        cub = np.zeros((n, 4, I, 3), np.float32)
        cub[self.n_layer:, 3, I - 1, 0] = SHIFT_PX * px                       # the last segment: SHIFT_PX to the right
        sigma = np.where(np.arange(n) < self.n_layer, 1.2, 0.6)[:, None]      # pixels
        scaling = np.log(np.concatenate([sigma * px, sigma * py, np.full((n, 1), 0.01)], 1)).astype(np.float32)
        rot = np.zeros((n, 4), np.float32)
        rot[:, 0] = 1.0
        host = dict(position=pos, pos_cubic_node=cub.reshape(n, -1), rotation=rot, rot_poly_feat=np.zeros((n, 4, 4), np.float32),
                    rot_fourier_feat=np.zeros((n, 8, 4), np.float32), opacity=np.full((n, 1), 8.0, np.float32), scaling=scaling)
        self.model = {k: _t(v) for k, v in host.items()}
        self.model["shs"] = _t(rng.normal(0, 0.3, size=(n, 16, 3)))
        self.extr = torch.eye(4, device="cuda")


def _grow(mask, r):
    """pixels within r (Chebyshev) of a True pixel"""
    m = torch.nn.functional.max_pool2d(mask[None, None].float(), 2 * r + 1, stride=1, padding=r)
    return m[0, 0] > 0


def test_known_occluder(gpu):
    from splatter_a_video_amd.flow import IN_FRONT, INCONSISTENT, OUTSIDE, render_flow
    from splatter_a_video_amd.views import render_views
    oc = Occluder()
    with torch.no_grad():
        rv = render_views(oc.model, oc.clock, [0.0, 29.0], oc.extr, W, H, frames_per_batch=2, cubic_layout=0)
        out = render_flow(oc.model, oc.clock, [0.0], [29.0], oc.extr, W, H, frames_per_batch=1, cubic_layout=0, occlusion=True,
                          cycle=True, depth_margin=0.5, min_coverage=0.5, fb_alpha=0.01, fb_beta=0.5)
    assert sorted(out) == ["coverage", "depth_gap", "fb_sq", "flow", "occlusion", "scene_flow", "track_depth", "warped"]
    depth1, depth2 = rv["depth"][0, 0], rv["depth"][1, 0]
    mask, gap, flow = out["occlusion"][0], out["depth_gap"][0], out["flow"][0]
    assert mask.dtype == torch.uint8 and mask.shape == (H, W) and out["warped"].shape == (1, 3, H, W) and out["fb_sq"].shape == (1, H, W)
    # the regions, from the depth renders alone
    A = (depth1 > 2.9) & (depth2 < 2.1)                                       # the background there is hidden at t2
    foot = (depth1 < 2.9) | (depth2 < 2.9)                                    # either footprint of the block
    B = (depth1 > 2.9) & (depth2 > 2.9) & ~_grow(foot, MARGIN_PX)
    C = depth1 < 2.1
    print(f"region A {int(A.sum())}, B {int(B.sum())}, C {int(C.sum())} pixels; depth1 {float(depth1.min()):.3f} .. {float(depth1.max()):.3f}")
    assert int(A.sum()) >= 100 and int(B.sum()) >= 100 and int(C.sum()) >= 100
    print(f"A: depth_gap {float(gap[A].min()):.3f} .. {float(gap[A].max()):.3f}; C: flow u {float(flow[0][C].min()):.3f} .. "
          f"{float(flow[0][C].max()):.3f}, |v| max {float(flow[1][C].abs().max()):.3e}; B: bits {int(mask[B].max())}")
    assert bool(((mask[A] & IN_FRONT) != 0).all()) and bool(((mask[A] & INCONSISTENT) != 0).all())
    assert bool(((gap[A] - 1.0).abs() <= 0.15).all())
    assert int(mask[B].max()) == 0
    assert not bool((mask[C] & IN_FRONT).any())
    assert bool((((flow[0][C] - SHIFT_PX) ** 2 + flow[1][C] ** 2).sqrt() <= 0.5).all())
    # frame t2's rgb pulled back to frame t1: the layer is static
    rgb1, warped = rv["rgb"][0], out["warped"][0]
    Bc = B[None].expand(3, H, W)
    err = (warped[Bc] - rgb1[Bc]).abs()
    print(f"warped against frame t1 on B: max err {float(err.max()):.3e}")
    assert torch.allclose(warped[Bc], rgb1[Bc], rtol=1e-4, atol=1e-5)
    outside = (mask & OUTSIDE) != 0
    assert int(_bits(warped[:, outside]).count_nonzero()) == 0
    # a flow that leaves the frame: OUTSIDE, and the pulled-back rgb exactly 0 there
    from splatter_a_video_amd.flow import flow_occlusion
    far = out["flow"].clone()
    far[:, 0, :, W - 8:] = 9.0
    occ = flow_occlusion(far, src=rv["rgb"][1:2])
    gone = (occ.mask[0] & OUTSIDE) != 0
    assert bool(gone[:, W - 8:].all()) and int(_bits(occ.warped[0][:, gone]).count_nonzero()) == 0
