"""camera_grad=True of FrameBatch.render_dynamic / render_dynamic_sets, end to end on the scene of tests/test_gpu_views.py (2001
dynamic Gaussians, 96 x 64, its cameras): extr.grad / intr.grad of the autograd node

1. against the float64 chain of tests/camera_grad_ref.py fed with the batch's OWN pair records (read back after the backward and
   segment-summed in float64 on the host): the node hands the kernel the right records, frames, strides and columns;
2. pinhole: against independent code -- the frame-by-frame composition dynamics.evaluate -> gs.project_point -> compute_cov3d ->
   ewa_project -> sort -> alpha_blending, whose project_point / ewa_project carry the reference's dL_dintr / dL_dextr (float
   atomics on that side: the bar, not bits);
3. the contract of the keyword;
4. descent: a step against dL/dxi through views.pose_delta lowers the image loss -- a transposed, wrongly scaled or wrongly
   signed gradient does not.

Bar: geometry_ref.Report.tensor (2e-3 |b| + 1e-4 max|b| per frame and tensor; over the sum for a shared camera)."""
import numpy as np
import pytest
import torch

import camera_grad_ref as cr
import geometry_ref as gr
import test_gpu_views as tv
from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import dynamics, views
from splatter_a_video_amd.frames import FrameBatch
from test_gpu_layers import H, N, NAMES, TIMES, W, Scene, _t

pytestmark = pytest.mark.gpu

K = tv.K
F = len(TIMES)
TRAIN = ("position", "pos_cubic_node", "rotation", "opacity", "scaling")
CAMERAS = ["ortho", "pinhole"]


@pytest.fixture(scope="module")
def scene(gpu):
    sc = Scene()
    sc.attr = _t(np.random.default_rng(23).uniform(-1, 1, size=(N, 2)))
    return sc


def _leaves(sc):
    return {k: sc.model[k].clone().requires_grad_(k in TRAIN) for k in NAMES}


def _camera(kind, per_frame_intr=True):
    """(extr [F,4,4], intr [F,4] / [4] / None, nearest) as device tensors"""
    if kind == "ortho":
        return _t(tv._cameras(F)), None, 0.01
    return _t(tv._cameras(F)), _t(tv._intr(F if per_frame_intr else None)), tv.NEAREST_PINHOLE


def _image_grads(widths, seed):
    rng = np.random.default_rng(seed)
    return [_t(rng.normal(size=(F, c, H, W))) for c in widths]


def _render_sets(sc, fb, extr, intr, nearest, camera_grad=True, **kw):
    lv = _leaves(sc)
    rgb = sc.rgb.clone().requires_grad_(True)
    sets = [dict(feature=rgb, bg=1.0, taps=True), dict(feature="depth", bg=1.0), dict(feature=sc.attr, bg=0.0, detach_opacity=True)]
    flags = dict(differentiable=True, camera_grad=True) if camera_grad else dict(differentiable=True)
    res = fb.render_dynamic_sets(sc.clock, TIMES, extr, sets, K=K, cubic_layout=0, intr=intr, nearest=nearest, **flags, **kw, **lv)
    return res, lv, rgb


def _backward_sets(sc, extr, intr, nearest, camera_grad=True, seed=3, fb=None, **kw):
    """one forward + backward of the three sets under random image gradients; returns (fb, leaves, rgb)"""
    fb = FrameBatch(F, N, W, H, 6, "cuda", want_abs=True) if fb is None else fb
    res, lv, rgb = _render_sets(sc, fb, extr, intr, nearest, camera_grad, **kw)
    outs = list(res[:-1])
    g = _image_grads((3, 1, 2), seed) + [torch.ones_like(t) for t in outs[3:]]
    torch.autograd.backward(outs, g)
    torch.cuda.synchronize()
    fb.check()
    return fb, lv, rgb


def _scene_case(sc, ortho, nearest):
    h = sc.host
    return dict(id="views_scene", clock=sc.clock, I=sc.I, N=N, W=W, H=H, ortho=ortho, nearest=nearest, extent=1.3,
                stratum=np.zeros(N, np.int64), position=h["position"], cubic=h["pos_cubic_node"], rotation=h["rotation"],
                rot_poly=h["rot_poly_feat"], rot_fourier=h["rot_fourier_feat"], scaling=h["scaling"])


def _record_reference(sc, fb, rec, stride, depth_column, extr, intr, nearest):
    """float64 camera gradients from the batch's own records: segment sums on the host, then camera_grad_ref's chain"""
    cap = fb.capacity
    rec = rec[:F * cap * stride].reshape(F, cap, stride).cpu().numpy().astype(np.float64)
    goff = fb.goff.cpu().numpy().astype(np.int64)
    c = _scene_case(sc, intr is None, nearest)
    extr_h = extr.detach().cpu().numpy()
    intr_h = None if intr is None else intr.detach().cpu().numpy().reshape(-1, 4)
    di, de, owners = [], [], 0
    for f, t in enumerate(TIMES):
        cnt = np.diff(np.concatenate([[0], goff[f]]))
        assert cnt.min() >= 0 and goff[f, -1] <= cap
        S = np.zeros((N, stride))
        np.add.at(S, np.repeat(np.arange(N), cnt), rec[f, :goff[f, -1]])
        idx = np.nonzero(cnt > 0)[0]
        owners += len(idx)
        g_d = S[:, depth_column:depth_column + 1] if depth_column >= 0 else np.zeros((N, 1))
        up = dict(g_uv=S[:, 0:2], g_conic=S[:, 2:5], g_d=g_d)
        k = np.zeros(4) if intr_h is None else intr_h[f if intr_h.shape[0] > 1 else 0]
        a, b = cr.frame_grads(c, k, extr_h[f] if extr_h.ndim == 3 else extr_h, t, up, idx, decide=False)
        di.append(a); de.append(b)
    assert owners > 1000 * F / 2
    return dict(intr=torch.stack(di), extr=torch.stack(de))


def _check(name, extr_grad, intr_grad, ref, share=False):
    rep = gr.Report(dict(id=name, N=N))
    e = extr_grad.detach().cpu().numpy()
    e = e[..., :3, :] if e.shape[-2] == 4 else e
    cr.check(rep, "", e.reshape(-1, 12) if not share else e.reshape(12), None if intr_grad is None else intr_grad.detach().cpu().numpy(),
             ref, share)
    rep.finish()


# ------------------------------------------------------------------ 1. the record route
@pytest.mark.parametrize("kind", CAMERAS)
def test_sets_records_reach_the_kernel(scene, kind):
    extr, intr, nearest = _camera(kind)
    extr.requires_grad_(True)
    if intr is not None:
        intr.requires_grad_(True)
    fb, lv, rgb = _backward_sets(scene, extr, intr, nearest)
    assert extr.grad.shape == extr.shape and not extr.grad[:, 3].any(), "the bottom row of a 4x4 gets zeros"
    assert float(extr.grad.abs().max()) > 0 and (intr is None or intr.grad.shape == intr.shape)
    stride = int(L.lib().splat_blend_sets_pair_stride(6))
    rec = fb._set_buffers[("rec", "sets")]
    ref = _record_reference(scene, fb, rec, stride, 12 + 3, extr, intr, nearest)
    _check(f"sets.{kind}", extr.grad, None if intr is None else intr.grad, ref)


@pytest.mark.parametrize("kind", CAMERAS)
def test_plain_records_reach_the_kernel(scene, kind):
    """render_dynamic: plain records (no depth column), extr [F,3,4]"""
    extr, intr, nearest = _camera(kind)
    extr = extr[:, :3].contiguous().requires_grad_(True)
    if intr is not None:
        intr.requires_grad_(True)
    fb = FrameBatch(F, N, W, H, 3, "cuda", want_abs=True)
    out = fb.render_dynamic(scene.clock, TIMES, extr, scene.rgb, bg=1.0, nearest=nearest, intr=intr, cubic_layout=0,
                            differentiable=True, camera_grad=True, **_leaves(scene))
    out.backward(_image_grads((3,), 77)[0])
    torch.cuda.synchronize()
    assert extr.grad.shape == (F, 3, 4)
    ref = _record_reference(scene, fb, fb.pair_records, fb.ncp, -1, extr, intr, nearest)
    assert not ref["extr"][:, 2, :3].any() or kind == "pinhole"        # no depth gradient: an orthographic third row gets nothing
    _check(f"plain.{kind}", extr.grad, None if intr is None else intr.grad, ref)


# ------------------------------------------------------------------ 2. pinhole: the per-operator path, frame by frame
def test_pinhole_against_the_per_operator_path(scene):
    import dptr.gs as gs
    sc = scene
    extr, intr, nearest = _camera("pinhole")
    extr.requires_grad_(True); intr.requires_grad_(True)
    g = _image_grads((3,), 41)[0]
    fb = FrameBatch(F, N, W, H, 3, "cuda")
    lv = _leaves(sc)
    out = fb.render_dynamic(sc.clock, TIMES, extr, sc.rgb, bg=1.0, nearest=nearest, intr=intr, cubic_layout=0, differentiable=True,
                            camera_grad=True, **lv)
    out.backward(g)
    e2 = extr.detach().clone().requires_grad_(True)
    k2 = intr.detach().clone().requires_grad_(True)
    lv2 = _leaves(sc)
    for f, t in enumerate(TIMES):
        pos, rot, opa, scl = dynamics.evaluate(sc.clock, t, **lv2)
        uv, depth = gs.project_point(pos, k2[f], e2[f], W, H, nearest, 1.3)
        vis = depth != 0
        cov = gs.compute_cov3d(scl, rot, vis)
        conic, radius, tiles = gs.ewa_project(pos, cov, k2[f], e2[f], uv, W, H, vis)
        idx, tr = gs.sort_gaussian(uv, depth, W, H, radius, tiles)
        img = gs.alpha_blending(uv, conic, opa, sc.rgb, idx, tr, 1.0, W, H, torch.zeros_like(uv, requires_grad=True))
        (img * g[f]).sum().backward()
    torch.cuda.synchronize()
    ref = dict(extr=e2.grad[:, :3].double().cpu(), intr=k2.grad.double().cpu())
    _check("per_operator", extr.grad, intr.grad, ref)


# ------------------------------------------------------------------ 3. the contract
def test_camera_grad_needs_differentiable(scene):
    fb = FrameBatch(F, N, W, H, 6, "cuda")
    extr, _, _ = _camera("ortho")
    sets = [dict(feature=scene.rgb, bg=1.0, taps=True), dict(feature="depth", bg=1.0), dict(feature=scene.attr, bg=0.0, detach_opacity=True)]
    with pytest.raises(ValueError, match="camera_grad=True needs differentiable=True"):
        fb.render_dynamic_sets(scene.clock, TIMES, extr, sets, cubic_layout=0, camera_grad=True, **_leaves(scene))
    fb3 = FrameBatch(F, N, W, H, 3, "cuda")
    with pytest.raises(ValueError, match="camera_grad=True needs differentiable=True"):
        fb3.render_dynamic(scene.clock, TIMES, extr[0], scene.rgb, cubic_layout=0, camera_grad=True, **_leaves(scene))
    with pytest.raises(ValueError, match="cameras are constants"):          # the default keeps refusing
        fb.render_dynamic_sets(scene.clock, TIMES, extr.clone().requires_grad_(True), sets, cubic_layout=0, differentiable=True,
                               **_leaves(scene))
    with pytest.raises(ValueError, match=r"grad_sink\['extr'\]"):
        fb.render_dynamic_sets(scene.clock, TIMES, extr, sets, cubic_layout=0, differentiable=True, camera_grad=True,
                               grad_sink={"extr": torch.zeros(F, 3, 4, device="cuda")}, **_leaves(scene))


@pytest.mark.parametrize("kind", CAMERAS + ["one_ortho"])
def test_parameter_gradients_keep_their_bits_and_no_camera_launches_nothing(scene, kind):
    extr, intr, nearest = _camera("ortho" if kind == "one_ortho" else kind)
    if kind == "one_ortho":
        extr = extr[2].contiguous()
    runs = []
    L.profile_enable(True)
    try:
        for mode in ("off", "on_constant", "on"):
            e = extr.clone().requires_grad_(mode == "on")
            L.profile_reset()
            fb, lv, rgb = _backward_sets(scene, e, intr, nearest, camera_grad=mode != "off")
            n = L.profile_read("cam_grad")[1]
            assert n == (0 if mode != "on" else (3 if kind == "one_ortho" else 2)), (mode, n)
            assert (L.profile_read("gauss_bwd_cam")[1] == 0) == (kind == "one_ortho")      # one [4,4] camera: the core twin
            runs.append({**{k: lv[k].grad.clone() for k in TRAIN}, "rgb": rgb.grad.clone(), "tap": fb.tap.clone(),
                         "abs_tap": fb.abs_tap.clone()})
            if mode == "on":
                assert e.grad is not None and float(e.grad.abs().max()) > 0
            else:
                assert e.grad is None
    finally:
        L.profile_enable(False)
    for k in runs[0]:
        assert float(runs[0][k].abs().max()) > 0, k
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k


def test_sinks_receive_the_gradients_by_addition(scene):
    extr, intr, nearest = _camera("pinhole", per_frame_intr=False)
    e, k = extr.clone().requires_grad_(True), intr.clone().requires_grad_(True)
    _backward_sets(scene, e, k, nearest)
    assert k.grad.shape == (4,)
    pre_e, pre_k = torch.full_like(extr, 0.5), torch.full_like(intr, -2.0)
    sink = {"extr": pre_e.clone(), "intr": pre_k.clone()}
    e2, k2 = extr.clone().requires_grad_(True), intr.clone().requires_grad_(True)
    _backward_sets(scene, e2, k2, nearest, grad_sink=sink)
    assert e2.grad is None and k2.grad is None
    assert torch.equal(sink["extr"], pre_e + e.grad) and torch.equal(sink["intr"], pre_k + k.grad)
    # a sink alone (nothing requires grad) still runs the kernel
    sink2 = {"extr": torch.zeros_like(extr)}
    _backward_sets(scene, extr, intr, nearest, grad_sink=sink2)
    assert torch.equal(sink2["extr"], e.grad)


@pytest.mark.parametrize("kind", CAMERAS)
def test_one_camera_receives_the_sum_over_the_frames(scene, kind):
    extr, intr, nearest = _camera(kind, per_frame_intr=False)
    one = extr[2].contiguous()
    eF = one[None].repeat(F, 1, 1).contiguous().requires_grad_(True)
    kF = None if intr is None else intr[None].repeat(F, 1).contiguous().requires_grad_(True)
    _backward_sets(scene, eF, kF, nearest)
    e1 = one.clone().requires_grad_(True)
    k1 = None if intr is None else intr.clone().requires_grad_(True)
    _backward_sets(scene, e1, k1, nearest)
    assert e1.grad.shape == (4, 4) and not e1.grad[3].any()
    ref = dict(extr=eF.grad[:, :3].double().cpu(), intr=None if kF is None else kF.grad.double().cpu())
    _check(f"shared.{kind}", e1.grad, None if k1 is None else k1.grad, ref, share=True)


@pytest.mark.parametrize("kind", CAMERAS)
def test_deterministic_mode_with_wide_points_and_ids(scene, kind):
    """camera_grad under splat_set_deterministic, with wide=, points=(ordered) and K > 0 present: twice, the same bits"""
    extr, intr, nearest = _camera(kind)
    rng = np.random.default_rng(12)
    counts = [8] * F
    xy = _t(np.stack([rng.integers(0, W, size=sum(counts)), rng.integers(0, H, size=sum(counts))], 1))
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device="cuda")
    wide = _t(rng.uniform(-1, 1, size=(N, 40)))
    runs = []
    L.set_deterministic(True)
    try:
        for _ in range(2):
            e = extr.clone().requires_grad_(True)
            k = None if intr is None else intr.clone().requires_grad_(True)
            fb = FrameBatch(F, N, W, H, 6, "cuda", want_abs=True)
            res, lv, rgb = _render_sets(scene, fb, e, k, nearest, wide=dict(feature=wide.clone().requires_grad_(True), bg=0.0,
                                                                            detach_opacity=True),
                                        points=dict(feature=scene.attr, points=xy, offsets=off, bg=0.0, detach_opacity=True, ordered=True))
            assert len(res) == 6 and res[-1].shape == (F, H, W, K)
            outs = list(res[:-1])
            g = _image_grads((3, 1, 2, 40), 8) + [torch.ones_like(outs[-1])]
            torch.autograd.backward(outs, g)
            torch.cuda.synchronize()
            runs.append((e.grad.clone(), None if k is None else k.grad.clone(), lv["position"].grad.clone()))
    finally:
        L.set_deterministic(False)
    for a, b in zip(*runs):
        assert (a is None and b is None) or (torch.equal(a, b) and float(a.abs().max()) > 0)
    # the wide and the sparse set's geometry terms are in the records the camera kernel reads: its gradient differs without them
    e0 = extr.clone().requires_grad_(True)
    _backward_sets(scene, e0, None if intr is None else intr.clone(), nearest, seed=8)
    assert not torch.equal(e0.grad, runs[0][0])


def test_in_place_edit_of_a_camera_is_caught(scene):
    """(the node saves the forward's camera tensor, which shares the leaf's version counter: autograd's own check answers in
    front of FrameBatch's, which words it "modified in place")"""
    extr, _, nearest = _camera("ortho")
    e = extr.clone().requires_grad_(True)
    fb = FrameBatch(F, N, W, H, 6, "cuda")
    res, lv, rgb = _render_sets(scene, fb, e, None, nearest)
    with torch.no_grad():
        e.mul_(1.0)
    with pytest.raises(RuntimeError, match="modified in place|modified by an inplace operation"):
        torch.autograd.backward(list(res[:3]), _image_grads((3, 1, 2), 3))


# ------------------------------------------------------------------ 4. descent
@pytest.mark.parametrize("kind", CAMERAS)
def test_a_step_against_the_pose_gradient_lowers_the_loss(scene, kind):
    sc = scene
    extr, intr, nearest = _camera(kind)
    fb = FrameBatch(F, N, W, H, 3, "cuda")
    lv = {k: sc.model[k] for k in NAMES}

    def render(e, **kw):
        return fb.render_dynamic(sc.clock, TIMES, e, sc.rgb, bg=1.0, nearest=nearest, intr=intr, cubic_layout=0, differentiable=True,
                                 **kw, **lv)
    with torch.no_grad():
        target = render(extr).clone()
    rng = np.random.default_rng(5)
    xi0 = _t(np.concatenate([rng.normal(0, 0.002, size=(F, 3)), rng.normal(0, 0.004, size=(F, 3))], 1))

    def loss(xi, grad=False):
        if grad:
            return ((render(views.pose_delta(extr, xi), camera_grad=True) - target) ** 2).sum()
        with torch.no_grad():
            return float(((render(views.pose_delta(extr, xi)) - target) ** 2).sum())
    xi = xi0.clone().requires_grad_(True)
    l0 = loss(xi, grad=True)
    l0.backward()
    l0 = l0.detach()
    g = xi.grad
    assert g.shape == (F, 6) and torch.isfinite(g).all() and float(g.norm()) > 0
    assert float(l0) > 0 and abs(loss(xi0) - float(l0)) <= 1e-5 * float(l0)
    s0 = 1e-2 / float(g.norm())
    tried = [loss(xi0 - s0 * 2.0 ** -k * g) for k in range(10)]
    print(f"{kind}: L(xi) = {float(l0):.6g}, L(xi - s g) for s = s0 2^-k: {['%.6g' % v for v in tried]}")
    assert min(tried) < float(l0)
    # the ascent direction does not lower it at the step that descends best: the sign is the gradient's
    k_best = int(np.argmin(tried))
    assert loss(xi0 + s0 * 2.0 ** -k_best * g) > tried[k_best]
