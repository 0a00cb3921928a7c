"""Dense optical flow on the GPU (splatter_a_video_amd.flow; csrc/flow.hip): the flow attribute of a batch of frame pairs and
its gradient against the float64 restatement of tests/flow_ref.py, ``render_flow`` against the frame batch fed with the
attribute (bits) and against the per-frame operators, the flow colours against the reference's own bytes
(tests/golden/flow_wheel.npz) and the flow error sums against float64.  Every bound is derived in tests/flow_ref.py."""
import os

import numpy as np
import pytest
import torch

import flow_ref as FR
from test_gpu_layers import H, N, NAMES, W, Scene, _dynamic_host, _t

pytestmark = pytest.mark.gpu

P = 601                                   # not a multiple of the 256-lane block
FRAMES = 30                               # knots at frames 0 4 9 14 19 24 29
PAIRS = {1: ([3.0], [12.5]),
         # inside one segment | inside one segment | fractional, inside | across segments | fractional | backwards | the whole clip
         7: ([0.0, 5.0, 6.5, 9.0, 14.0, 22.25, 29.0], [2.0, 8.0, 7.75, 20.0, 14.5, 21.0, 0.0])}
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "flow_wheel.npz")
CASES = ("random", "odd", "zeros", "directions", "stack", "clip", "bgr")


def _rot(ax, a):
    c, s = np.cos(a), np.sin(a)
    R = np.eye(4, dtype=np.float32)
    i, j = [(1, 2), (0, 2), (0, 1)][ax]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _extr(k):
    e = (_rot(0, 0.05 * np.sin(1.0 + 2.0 * k)) @ _rot(2, 0.09 * np.cos(0.5 + 1.3 * k))).astype(np.float32)
    e[:3, 3] = (0.05 * np.sin(0.7 * k), -0.04 * np.cos(1.1 * k), 0.2 + 0.1 * np.sin(0.4 * k))
    return e


def _cameras(kind, F):
    """(extr, intr, extr2, intr2, nearest) as numpy"""
    k = np.array([84.0, 80.0, W / 2 + 0.75, H / 2 - 0.5], np.float32)
    if kind == "ortho":
        return _extr(0), None, None, None, 0.01
    if kind == "ortho_per_pair":
        return np.stack([_extr(f) for f in range(F)]), None, None, None, 0.01
    if kind == "pinhole":
        return np.stack([_extr(f) for f in range(F)]), np.stack([k * (1 + 0.02 * np.sin(f)) for f in range(F)]).astype(np.float32), \
            None, None, 0.2
    if kind == "extr2":
        return _extr(0), None, np.stack([_extr(3 + f) for f in range(F)]), None, 0.01
    if kind == "pinhole_extr2":
        return _extr(1), k, _extr(2), (k * np.array([1.05, 0.97, 1.0, 1.0], np.float32)).astype(np.float32), 0.2
    raise KeyError(kind)


@pytest.fixture(scope="module")
def model(gpu):
    clock, host, _ = _dynamic_host(P, FRAMES, 11)
    return clock, host


def _attr_call(clock, host, t1, t2, cams, layout=0, zero=False, **kw):
    from splatter_a_video_amd.dynamics import to_segment_major
    from splatter_a_video_amd.flow import flow_attribute
    e, i_, e2, i2, nearest = cams
    opt = lambda a: None if a is None else _t(a)
    pos = kw.pop("position", None)
    cub = kw.pop("cubic", None)
    pos = _t(host["position"]) if pos is None else pos
    if cub is None:
        cub = _t(host["pos_cubic_node"])
        cub = to_segment_major(cub, clock.interval_num) if layout == 1 else cub
    return flow_attribute(clock, t1, t2, _t(e), W, H, position=pos, pos_cubic_node=cub, intr=opt(i_), extr2=opt(e2), intr2=opt(i2),
                          cubic_layout=layout, nearest=nearest, zero_culled=zero, **kw)


def _ref(clock, host, t1, t2, cams, zero=False, g=None, position=None, cubic=None):
    e, i_, e2, i2, nearest = cams
    return FR.attribute(clock, t1, t2, host["position"] if position is None else position,
                        host["pos_cubic_node"] if cubic is None else cubic, e, i_, e2, i2, W, H, nearest, 1.3, zero, g=g)


# ------------------------------------------------------------------ 1. attribute, forward
@pytest.mark.parametrize("F", [1, 7])
@pytest.mark.parametrize("kind", ["ortho", "ortho_per_pair", "pinhole", "extr2", "pinhole_extr2"])
def test_attribute_forward_against_float64(model, kind, F):
    clock, host = model
    t1, t2 = PAIRS[F]
    cams = _cameras(kind, F)
    ref = _ref(clock, host, t1, t2, cams)
    got = _attr_call(clock, host, t1, t2, cams).cpu().numpy().astype(np.float64)
    seg = _attr_call(clock, host, t1, t2, cams, layout=1).cpu().numpy()
    assert got.shape == (F, P, 2)
    assert np.array_equal(seg.view(np.int32), got.astype(np.float32).view(np.int32))        # both layouts: the same arithmetic
    keep = ~ref["near"]
    gam = FR.gamma(ref)
    err = np.abs(got - ref["flow"])
    bound = gam * (np.abs(ref["uv1"]) + np.abs(ref["uv2"]) + 1.0)
    print(f"{kind} F={F}: gamma {gam:.3e}, left out {1 - keep.mean():.3%}, culled at t1 {ref['cull1'].mean():.3%}, "
          f"max err / bound {float((err / bound)[keep].max()):.3f}, max |flow| {np.abs(ref['flow']).max():.2f} px")
    assert 1 - keep.mean() <= 0.01
    assert gam < 1e-3                       # N_ROUND EPS kappa with kappa < 800: the chain's terms are a few hundred pixels at the most
    assert (err <= bound)[keep].all()
    assert np.abs(ref["flow"]).max() > 1.0                               # the scene moves


def _hand_placed(clock):
    """five Gaussians that do not move inside a segment (only the constant coefficient c3 of a segment is set): at time 0
    (segment 0) and time 29 (the last segment) they sit where the case wants them"""
    I = clock.interval_num
    pos = np.tile(np.array([[0.2, -0.1, 3.0]], np.float32), (5, 1))
    cub = np.zeros((5, 4, I, 3), np.float32)
    cub[0, 3, 0] = (2.5, 0.0, 0.0)        # 0: outside the extent at t1 only
    cub[1, 3, I - 1] = (0.0, -2.6, 0.0)   # 1: outside the extent at t2 only
    cub[2, 3, :] = (0.0, 0.0, -4.0)       # 2: behind the camera at both
    cub[3, 3, :] = (0.0, 0.0, -2.9)       # 3: depth 0.1: in front of the camera, nearer than `nearest` of either camera kind
    cub[3, 3, I - 1] = (0.3, 0.1, 0.0)    #    ... at t1 only: the near plane alone culls it
    cub[4, 3, :] = (-2.7, 0.0, 0.0)       # 4: outside the extent at both
    return pos, cub.reshape(5, -1)


@pytest.mark.parametrize("kind", ["ortho", "pinhole_extr2"])
def test_hand_placed_cull_decisions(gpu, kind):
    from splatter_a_video_amd.dynamics import FrameClock
    clock = FrameClock(FRAMES)
    pos, cub = _hand_placed(clock)
    e, i_, e2, i2, _ = _cameras(kind, 1)
    e = np.eye(4, dtype=np.float32)
    cams = (e, i_, None if e2 is None else e, i2, 0.3)
    for zero in (False, True):
        ref = _ref(clock, None, [0.0], [29.0], cams, zero=zero, position=pos, cubic=cub)
        assert ref["cull1"][0].tolist() == [True, False, True, True, True] and ref["cull2"][0].tolist() == [False, True, True, False, True]
        assert not ref["near"].any()
        got = _attr_call(clock, None, [0.0], [29.0], cams, zero=zero, position=_t(pos), cubic=_t(cub)).cpu().numpy()[0]
        for n in range(5):
            c1, c2 = ref["cull1"][0, n], ref["cull2"][0, n]
            if (c1 and c2) or (zero and (c1 or c2)):
                assert got[n].view(np.int32).tolist() == [0, 0], (kind, zero, n)               # +0.0
            else:
                want = ref["uv2"][0, n] if c1 else -ref["uv1"][0, n]                           # uv2 or -uv1, never a difference
                assert np.all(want != 0) and np.allclose(got[n], want, rtol=1e-5, atol=1e-4), (kind, zero, n, got[n], want)


@pytest.mark.parametrize("kind", ["ortho_per_pair", "pinhole"])
def test_identical_pairs_are_plus_zero(model, kind):
    clock, host = model
    t1, _ = PAIRS[7]
    for layout in (0, 1):
        out = _attr_call(clock, host, t1, t1, _cameras(kind, 7), layout=layout)
        assert int(out.view(torch.int32).count_nonzero()) == 0


def test_positions_are_positions_batch_bits(model):
    """an orthographic identity camera makes uv an affine map of the position: rebuilt in torch (every step rounded once) from
    positions_batch's own output it has to give the kernel's bits"""
    from splatter_a_video_amd.dynamics import frame_table, positions_batch_forward, to_segment_major
    clock, host = model
    t1, t2 = PAIRS[7]
    eye = np.eye(4, dtype=np.float32)
    for layout in (0, 1):
        cub = _t(host["pos_cubic_node"])
        cub = to_segment_major(cub, clock.interval_num) if layout else cub
        uv = []
        for t in (t1, t2):
            p = positions_batch_forward(frame_table(clock, t, "cuda"), _t(host["position"]), cub, clock.interval_num, layout)
            uv.append(torch.stack([((p[..., 0] + 1.0) * float(W)) / 2.0 - 0.5, ((p[..., 1] + 1.0) * float(H)) / 2.0 - 0.5], -1))
            assert float(p[..., 2].min()) > 1.0 and float(uv[-1][..., 0].abs().max()) < 1.1 * W     # nothing is culled
        got = _attr_call(clock, host, t1, t2, (eye, None, None, None, 0.01), layout=layout)
        assert torch.equal(got, uv[1] - uv[0])


# ------------------------------------------------------------------ 2. attribute, backward
def _grad_close(a, b, name):
    """the project's gradient parity: element-wise rtol 2e-3 + 1e-4 of the tensor's maximum"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    mx = max(float(np.abs(b).max()), 1e-30)
    err = np.abs(a - b)
    print(f"{name}: max err {err.max():.3e} of max {mx:.3e}")
    assert (err <= 2e-3 * np.abs(b) + 1e-4 * mx).all(), name


def _direct_backward(clock, host_t, t1, t2, cams, g, layout=0, zero=False, accumulate=False, bufs=None):
    from splatter_a_video_amd.dynamics import frame_table
    from splatter_a_video_amd.flow import _pair_cameras, flow_attribute_backward
    e, i_, e2, i2, nearest = cams
    opt = lambda a: None if a is None else _t(a)
    cam1, cam2 = _pair_cameras(_t(e), opt(i_), opt(e2), opt(i2), len(t1))
    pos, cub = host_t
    d_pos, d_cub = bufs if bufs is not None else (torch.full_like(pos, 7.0), torch.full_like(cub, -3.0))   # overwritten
    flow_attribute_backward(frame_table(clock, t1, "cuda"), frame_table(clock, t2, "cuda"), pos, cub, clock.interval_num, layout, cam1,
                            cam2, W, H, nearest, 1.3, zero, g, accumulate, d_pos, d_cub)
    return d_pos, d_cub


@pytest.mark.parametrize("kind", ["ortho", "ortho_per_pair", "pinhole", "extr2", "pinhole_extr2"])
def test_attribute_backward_against_float64(model, kind):
    from splatter_a_video_amd import _lib as L
    from splatter_a_video_amd.dynamics import to_gaussian_major, to_segment_major
    clock, host = model
    I = clock.interval_num
    t1, t2 = PAIRS[7]
    cams = _cameras(kind, 7)
    rng = np.random.default_rng(3)
    g = rng.normal(size=(7, P, 2)).astype(np.float32)
    ref = _ref(clock, host, t1, t2, cams, g=g)
    pos, cub = _t(host["position"]), _t(host["pos_cubic_node"])
    d_pos, d_cub = _direct_backward(clock, (pos, cub), t1, t2, cams, _t(g))
    _grad_close(d_pos.cpu().numpy(), ref["d_position"], f"{kind} d_position")
    _grad_close(d_cub.cpu().numpy(), ref["d_cubic"], f"{kind} d_pos_cubic_node")
    # two runs, the second in deterministic mode: the same bits
    L.set_deterministic(True)
    try:
        again = _direct_backward(clock, (pos, cub), t1, t2, cams, _t(g))
    finally:
        L.set_deterministic(False)
    assert torch.equal(again[0], d_pos) and torch.equal(again[1], d_cub)
    # the native layout: the same sums in the same order
    seg = _direct_backward(clock, (pos, to_segment_major(cub, I)), t1, t2, cams, _t(g), layout=1)
    assert torch.equal(seg[0], d_pos) and torch.equal(to_gaussian_major(seg[1].reshape(I, P, 4, 3)), d_cub)
    # accumulate adds to what the buffers hold
    pre = (torch.full_like(pos, 0.5), torch.full_like(cub, -0.25))
    acc = _direct_backward(clock, (pos, cub), t1, t2, cams, _t(g), accumulate=True, bufs=(pre[0].clone(), pre[1].clone()))
    assert torch.equal(acc[0], pre[0] + d_pos)
    assert torch.allclose(acc[1], pre[1] + d_cub, rtol=1e-6, atol=1e-6 * float(d_cub.abs().max()))
    # autograd through flow_attribute is the direct call; a sink receives the same by addition
    pa, ca = pos.clone().requires_grad_(True), cub.clone().requires_grad_(True)
    _attr_call(clock, host, t1, t2, cams, position=pa, cubic=ca).backward(_t(g))
    assert torch.equal(pa.grad, d_pos) and torch.equal(ca.grad, d_cub)
    pb, cb = pos.clone().requires_grad_(True), cub.clone().requires_grad_(True)
    sink = dict(position=torch.zeros_like(pos), pos_cubic_node=torch.zeros_like(cub))
    _attr_call(clock, host, t1, t2, cams, position=pb, cubic=cb, grad_sink=sink).backward(_t(g))
    assert pb.grad is None and cb.grad is None and torch.equal(sink["position"], d_pos) and torch.equal(sink["pos_cubic_node"], d_cub)


@pytest.mark.parametrize("zero", [False, True])
def test_backward_culled_sides_get_exactly_zero(gpu, zero):
    from splatter_a_video_amd.dynamics import FrameClock
    clock = FrameClock(FRAMES)
    I = clock.interval_num
    pos, cub = _hand_placed(clock)
    cams = (np.eye(4, dtype=np.float32), None, None, None, 0.3)
    g = np.array([[[1.5, -2.0]] * 5], np.float32)
    ref = _ref(clock, None, [0.0], [29.0], cams, zero=zero, g=g, position=pos, cubic=cub)
    d_pos, d_cub = _direct_backward(clock, (_t(pos), _t(cub)), [0.0], [29.0], cams, _t(g), zero=zero)
    d_pos, d_cub = d_pos.cpu().numpy(), d_cub.cpu().numpy().reshape(5, 4, I, 3)
    _grad_close(d_pos, ref["d_position"], "hand-placed d_position")
    _grad_close(d_cub, ref["d_cubic"], "hand-placed d_pos_cubic_node")
    assert (d_cub[:, :, 1:I - 1] == 0).all()                              # segments no pair touches
    for n, (c1, c2) in enumerate(zip(ref["cull1"][0], ref["cull2"][0])):
        dead1, dead2 = c1 or (zero and c2), c2 or (zero and c1)
        assert (d_cub[n, :, 0] == 0).all() == bool(dead1), n
        assert (d_cub[n, :, I - 1] == 0).all() == bool(dead2), n
        if dead1 and dead2:
            assert (d_pos[n] == 0).all(), n


# ------------------------------------------------------------------ 3. render_flow
T_CLIP = ([0.0, 3.0, 6.5, 14.0, 22.0], [2.0, 9.0, 8.25, 12.0, 29.0])


@pytest.fixture(scope="module")
def scene(gpu):
    sc = Scene()
    sc.geo = {k: sc.model[k] for k in NAMES}
    return sc


def _render(sc, **kw):
    from splatter_a_video_amd.flow import render_flow
    with torch.no_grad():
        return render_flow(dict(sc.model), sc.clock, T_CLIP[0], T_CLIP[1], sc.extr, W, H, frames_per_batch=2, cubic_layout=0, **kw)


def test_render_flow_is_the_frame_batch_fed_with_the_attribute(scene):
    from splatter_a_video_amd.flow import flow_attribute
    from splatter_a_video_amd.frames import FrameBatch
    sc = scene
    st = {}
    out = _render(sc, coverage=True, stats=st)
    assert sorted(out) == ["coverage", "flow"] and out["flow"].shape == (5, 2, H, W) and out["coverage"].shape == (5, 1, H, W)
    assert st["regrows"] == 0 and not out["flow"].requires_grad
    fb = FrameBatch(2, N, W, H, 3, "cuda", records=False)
    ones = torch.ones(N, 1, device="cuda")
    pad = [0, 1, 2, 3, 4, 4]
    with torch.no_grad():
        for b0 in (0, 2, 4):
            t1, t2 = [T_CLIP[0][i] for i in pad[b0:b0 + 2]], [T_CLIP[1][i] for i in pad[b0:b0 + 2]]
            attr = flow_attribute(sc.clock, t1, t2, sc.extr, W, H, position=sc.geo["position"], pos_cubic_node=sc.geo["pos_cubic_node"])
            row = fb.render_dynamic_sets(sc.clock, t1, sc.extr, [dict(feature=[attr, ones], bg=0.0, detach_opacity=True)],
                                         cubic_layout=0, **sc.geo)[0]
            fb.check()
            n = min(2, 5 - b0)
            assert torch.equal(out["flow"][b0:b0 + n], row[:n, :2]) and torch.equal(out["coverage"][b0:b0 + n], row[:n, 2:3])
    assert float(out["flow"].abs().max()) > 1.0 and 0.5 < float(out["coverage"].max()) <= 1.0 + 1e-5
    # flow alone, and beside the video row: the same flow within the image rule (another plan of the same compositing)
    alone = _render(sc)
    assert sorted(alone) == ["flow"] and torch.allclose(alone["flow"], out["flow"], rtol=1e-4, atol=1e-5 * float(out["flow"].abs().max()))
    video = _render(sc, with_video=True, coverage=True)
    assert sorted(video) == ["coverage", "depth", "flow", "mask_attribute", "rgb"] and video["rgb"].shape == (5, 3, H, W)
    assert torch.allclose(video["flow"], out["flow"], rtol=1e-4, atol=1e-5 * float(out["flow"].abs().max()))
    from splatter_a_video_amd.views import render_views
    rv = render_views(dict(sc.model), sc.clock, T_CLIP[0], sc.extr, W, H, frames_per_batch=2, cubic_layout=0)
    for k in ("rgb", "depth", "mask_attribute"):
        assert torch.allclose(video[k], rv[k], rtol=1e-4, atol=1e-5), k


def _reference_flow(sc, geo, t1, t2, extr, want_cov=False):
    """the reference's expression from the per-frame operators: project_point at both times, the difference composited by
    gs.alpha_blending with the opacity detached and background 0 over the sort of frame t1"""
    import dptr.gs as gs
    from splatter_a_video_amd.dynamics import evaluate, frame_preprocess
    imgs, attrs = [], []
    for a, b in zip(t1, t2):
        uv, depth, conic, radius, tiles, opa = frame_preprocess(sc.clock, a, extr, W, H, **geo, nearest=0.01, cubic_layout=0)
        idx, tr = gs.sort_gaussian(uv, depth, W, H, radius, tiles)
        uvs = []
        for t in (a, b):
            pos_t = evaluate(sc.clock, t, position=geo["position"], pos_cubic_node=geo["pos_cubic_node"], cubic_layout=0)[0]
            uvs.append(gs.project_point_ortho(pos_t, extr, W, H, 0.01, 1.3)[0])
        attr = uvs[1] - uvs[0]
        feat = torch.cat([attr, torch.ones_like(attr[:, :1])], 1) if want_cov else attr
        imgs.append(gs.alpha_blending(uv, conic, opa.detach(), feat, idx, tr, 0.0, W, H))
        attrs.append(attr.detach())
    return torch.stack(imgs), torch.stack(attrs)


def test_render_flow_against_the_per_frame_operators(scene):
    sc = scene
    out = _render(sc, coverage=True)
    with torch.no_grad():
        ref, attrs = _reference_flow(sc, sc.geo, T_CLIP[0], T_CLIP[1], sc.extr, want_cov=True)
    mx = float(attrs.abs().max())
    got = torch.cat([out["flow"], out["coverage"]], 1)
    bad = ((got - ref).abs() > 1e-5 * mx + 1e-4 * ref.abs())
    print(f"max |attr| {mx:.2f} px, outside the scaled image rule: {float(bad.float().mean()):.2e}, max err {float((got - ref).abs().max()):.3e}")
    assert mx > 1.0 and not bool(bad.any())


def test_render_flow_regrows_a_small_capacity(scene):
    st = {}
    small = _render(scene, capacity=64, stats=st)
    assert st["regrows"] >= 1 and st["capacity"] > 1000
    assert torch.equal(small["flow"], _render(scene)["flow"])


def test_render_flow_differentiable_and_forward_only_contract(scene):
    from splatter_a_video_amd.flow import render_flow
    sc = scene
    rng = np.random.default_rng(8)
    g = _t(rng.normal(size=(5, 2, H, W)))
    live = lambda: dict(sc.model, position=sc.model["position"].clone().requires_grad_(True),
                        pos_cubic_node=sc.model["pos_cubic_node"].clone().requires_grad_(True))
    with pytest.raises(ValueError, match="forward only"):
        render_flow(live(), sc.clock, T_CLIP[0], T_CLIP[1], sc.extr, W, H, frames_per_batch=2, cubic_layout=0)
    grads = []
    for _ in range(2):
        m = live()
        out = render_flow(m, sc.clock, T_CLIP[0], T_CLIP[1], sc.extr, W, H, frames_per_batch=2, cubic_layout=0, differentiable=True)
        assert out["flow"].requires_grad
        out["flow"].backward(g)
        grads.append((m["position"].grad, m["pos_cubic_node"].grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])            # run to run: the same bits
    with torch.no_grad():
        assert torch.equal(out["flow"].detach(), _render(sc)["flow"])
    m = live()
    geo = {k: m[k] for k in NAMES}
    ref, _ = _reference_flow(sc, geo, T_CLIP[0], T_CLIP[1], sc.extr)
    ref.backward(g)
    _grad_close(grads[0][0].cpu().numpy(), m["position"].grad.cpu().numpy(), "render_flow d_position")
    _grad_close(grads[0][1].cpu().numpy(), m["pos_cubic_node"].grad.cpu().numpy(), "render_flow d_pos_cubic_node")


# ------------------------------------------------------------------ 4. colours
def _maps(flow):
    f = flow if flow.ndim == 4 else flow[None]
    return np.ascontiguousarray(np.moveaxis(f, -1, 1))


@pytest.mark.parametrize("name", CASES)
def test_colours_against_the_reference_bytes(gpu, name):
    from splatter_a_video_amd.flow import flow_to_image
    g = np.load(GOLDEN)
    flow, img = _maps(g[name + "_flow"]), g[name + "_img"]
    img = img if img.ndim == 4 else img[None]
    scale = "whole_clip" if g[name + "_flow"].ndim == 4 else "per_frame"
    clip = 2.5 if name == "clip" else None
    got, rad = flow_to_image(_t(flow), clip_flow=clip, scale=scale, convert_to_bgr=name == "bgr", return_scale=True)
    got = got.cpu().numpy()
    assert got.shape == img.shape and got.dtype == np.uint8
    _, pre, exact, margin, _ = FR.colours(flow, clip_flow=clip, scale=scale, bgr=name == "bgr")
    dec = FR.decided(pre, exact, margin)
    diff = got.astype(np.int32) - img.astype(np.int32)
    print(f"{name}: {int((diff != 0).sum())} of {diff.size} bytes differ from the reference's, undecided {1 - dec.mean():.3%}, "
          f"exact 255: {exact.mean():.3%}")
    assert np.abs(diff).max() <= 1
    assert not (diff != 0)[dec].any()
    assert 1 - dec.mean() <= 0.05
    # the scale is the float32 maximum radius, exactly
    f32 = np.clip(flow, 0, np.float32(clip)) if clip else flow
    r32 = np.sqrt(np.square(f32[:, 0]) + np.square(f32[:, 1]))
    want = np.full(flow.shape[0], r32.max()) if scale == "whole_clip" else r32.reshape(flow.shape[0], -1).max(1)
    assert rad.cpu().numpy().view(np.int32).tolist() == want.astype(np.float32).view(np.int32).tolist()


def test_colours_given_scale_beyond_the_wheel_and_non_finite(gpu):
    from splatter_a_video_amd.flow import flow_to_image
    rng = np.random.default_rng(4)
    flow = rng.normal(0, 3.0, size=(2, 2, 37, 53)).astype(np.float32)
    got, rad = flow_to_image(_t(flow), scale=2.0, return_scale=True)
    got = got.cpu().numpy()
    img, pre, exact, margin, _ = FR.colours(flow, scale=2.0)
    beyond = np.sqrt(flow[:, 0].astype(np.float64) ** 2 + flow[:, 1] ** 2) > 2.0 + 1e-3
    assert 0.2 < beyond.mean() < 0.9 and rad.cpu().tolist() == [2.0, 2.0]
    dec = FR.decided(pre, exact, margin)
    diff = got.astype(np.int32) - img.astype(np.int32)
    print(f"given scale: {int((diff != 0).sum())} bytes differ, undecided {1 - dec.mean():.3%}, beyond the wheel {beyond.mean():.1%}")
    assert np.abs(diff).max() <= 1 and not (diff != 0)[dec].any() and 1 - dec.mean() <= 0.05
    assert (got[beyond].max(-1) <= 191).all()                            # col * 0.75: no channel above floor(255 * 0.75)
    # a non-finite pixel is black and does not poison the maximum
    bad = flow.copy()
    bad[0, 0, 3, 5], bad[0, 1, 7, 9], bad[1, 0, 0, 0] = np.nan, np.inf, -np.inf
    clean = flow.copy()
    clean[0, :, 3, 5] = clean[0, :, 7, 9] = clean[1, :, 0, 0] = 0.0
    for scale in ("per_frame", "whole_clip"):
        a, ra = flow_to_image(_t(bad), scale=scale, return_scale=True)
        b, rb = flow_to_image(_t(clean), scale=scale, return_scale=True)
        assert torch.equal(ra, rb) and bool(torch.isfinite(ra).all())
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert (a[0, 3, 5] == 0).all() and (a[0, 7, 9] == 0).all() and (a[1, 0, 0] == 0).all() and (b[0, 3, 5] == 255).all()
        a[0, 3, 5] = a[0, 7, 9] = a[1, 0, 0] = 255
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ 5. error
def test_flow_error_sums_gradient_and_zero_weight_frame(gpu):
    from splatter_a_video_amd.flow import flow_epe, flow_error_sums
    from splatter_a_video_amd.losses import flow_l1
    rng = np.random.default_rng(6)
    Hs, Ws = 37, 53                                                       # 1961 pixels: one partial of n = 1961 <= 2048 terms per map
    pred = rng.normal(0, 2.0, size=(3, 2, Hs, Ws)).astype(np.float32)
    gt = rng.normal(0, 2.0, size=(3, 2, Hs, Ws)).astype(np.float32)
    gt[0, :, :4] = pred[0, :, :4]                                         # exact zeros of the difference: sign(0) = 0
    w = rng.uniform(size=(3, Hs, Ws)).astype(np.float32)
    w[1] = 0.0
    sums_ref, grad_ref = FR.error_sums(pred, gt, w, scale=0.7)
    sums, grad = flow_error_sums(_t(pred), _t(gt), _t(w), scale=0.7, want_grad=True)
    again = flow_error_sums(_t(pred), _t(gt), _t(w), scale=0.7, want_grad=True)
    assert torch.equal(sums, again[0]) and torch.equal(grad, again[1])    # two runs: the same bits
    sums, grad = sums.cpu().numpy(), grad.cpu().numpy()
    assert Hs * Ws <= FR.PARTIAL_N
    bound = FR.SUM_ROUNDINGS * FR.EPS * sums_ref
    print("sums", sums.tolist(), "err / bound", (np.abs(sums - sums_ref) / np.maximum(bound, 1e-300)).tolist())
    assert (np.abs(sums - sums_ref) <= bound).all()
    assert (sums[1] == 0).all() and (grad[1] == 0).all() and not np.isnan(grad).any()
    # the kernel divides by ITS sum of the weights (SUM_ROUNDINGS); the float32 scale, scale / sum w and the product with w round
    # once each
    assert (np.abs(grad - grad_ref) <= (FR.SUM_ROUNDINGS + 4) * FR.EPS * np.abs(grad_ref)).all()
    assert (grad[0, :, :4] == 0).all() and np.abs(grad[0, :, 4:]).min() > 0
    # the public surface
    p = _t(pred).requires_grad_(True)
    loss = flow_l1(p, _t(gt), _t(w))
    want = float((sums_ref[:, 0] / np.maximum(sums_ref[:, 2], 1e-30)).mean())
    assert abs(float(loss) - want) <= 1e-5 * want
    (2.0 * loss).backward()
    _, g3 = FR.error_sums(pred, gt, w, scale=2.0 / 3.0)
    assert np.allclose(p.grad.cpu().numpy(), g3, rtol=1e-5, atol=0) and (p.grad[1] == 0).all()
    epe = flow_epe(_t(pred), _t(gt), _t(w)).cpu().numpy()
    assert np.allclose(epe, sums_ref[:, 1] / np.maximum(sums_ref[:, 2], 1e-30), rtol=1e-5) and epe[1] == 0
    assert flow_epe(_t(pred), _t(pred)).tolist() == [0.0, 0.0, 0.0]
    unweighted, _ = flow_error_sums(_t(pred), _t(gt))
    assert unweighted[:, 2].tolist() == [float(Hs * Ws)] * 3
