"""Training a dynamic frame batch under cameras per frame and the pinhole camera (render_dynamic / render_dynamic_sets with
differentiable=True: the batched forward of include/splat_hip_views.h, the unchanged tile backward, the Gaussian-side backward
of include/splat_hip_views_grad.h), end to end on the scene of tests/test_gpu_views.py: 2001 dynamic Gaussians, 96 x 64, the
sets rgb with taps | depth | 2 detached attributes, K = 4, random image gradients.

1. against the CPU oracle frame by frame (tests/oracle_chain_cam.py): images and geometry by the rules of
   test_gpu_views._check_against_oracle, every parameter, feature, tap and abs_tap gradient by assert_grad at GRAD_RTOL when the
   radii agree everywhere and 5e-3 otherwise (the rule of test_render_dynamic_sets_against_oracle_with_reference_parameters);
2. F equal copies of one orthographic camera as [F,4,4] (the new kernels) against the same camera as [4,4] (the one-camera
   path), with everything the one-camera path takes: a per-frame [F,P,3] tensor in the attribute set, wide=, points= (atomic
   and ordered), grad_sink for a parameter and a feature.  Not bits: the two forward kernels may contract differently;
3. the contract: one [4,4] camera with differentiable=True is the default path bit for bit, cameras that require grad raise,
   the default still refuses, two backward passes give the same bits, the deterministic-mode rule of points=."""
import numpy as np
import pytest
import torch

import oracle_chain_cam as occ
import test_gpu_views as tv
from splatter_a_video_amd import _lib as L
from splatter_a_video_amd.frames import FrameBatch
from test_gpu_frames_oracle import _same_geometry
from test_gpu_layers import H, N, NAMES, TIMES, W, Scene, _t
from test_gpu_parity import GRAD_RTOL, IMG_ATOL, IMG_RTOL, assert_grad

pytestmark = pytest.mark.gpu

K = tv.K
TRAIN = ("position", "pos_cubic_node", "rotation", "opacity", "scaling")


@pytest.fixture(scope="module")
def scene(gpu):
    sc = Scene()
    rng = np.random.default_rng(23)
    sc.attr_np = rng.uniform(-1, 1, size=(N, 2)).astype(np.float32)
    sc.attr = _t(sc.attr_np)
    return sc


def _leaves(sc):
    return {k: sc.model[k].clone().requires_grad_(k in TRAIN) for k in NAMES}


def _image_grads(F, widths, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(F, c, H, W)).astype(np.float32) for c in widths]


def _check_param_grads(lv, tot, tol, I):
    assert_grad(lv["pos_cubic_node"].grad.reshape(N, 4, I, 3), tot["pos_cubic_node"], "pos_cubic_node", tol)
    for k in ("position", "rotation", "opacity", "scaling"):
        assert_grad(lv[k].grad, tot[k], k, tol)


# ------------------------------------------------------------------ 1. against the oracle, frame by frame
def _sets_against_oracle(o, sc, times, extr, intr, nearest, name, min_pairs):
    F = len(times)
    fb = FrameBatch(F, N, W, H, 6, "cuda", want_abs=True)
    lv = _leaves(sc)
    rgb, attr = sc.rgb.clone().requires_grad_(True), sc.attr.clone().requires_grad_(True)
    sets = [dict(feature=rgb, bg=1.0, taps=True), dict(feature="depth", bg=1.0), dict(feature=attr, bg=0.0, detach_opacity=True)]
    res = fb.render_dynamic_sets(sc.clock, times, _t(extr), sets, K=K, nearest=nearest, intr=None if intr is None else _t(intr),
                                 cubic_layout=0, differentiable=True, **lv)
    assert all(t.requires_grad for t in res[:3]) and not res[-1].requires_grad
    gs_ = _image_grads(F, (3, 1, 2), 31 + F)
    torch.autograd.backward(list(res[:3]), [_t(g) for g in gs_])
    torch.cuda.synchronize()
    fb.check()
    per, tot = occ.dynamic_frames_cam(o, sc.clock, times, sc.host, extr, intr, W, H, tv._np_sets(sc), gs_, K, nearest)
    tv._check_against_oracle(fb, tuple(t.detach() for t in res[:3]) + (res[-1],), per, name, min_pairs)
    tol = GRAD_RTOL if _same_geometry(fb, per) else 5e-3
    _check_param_grads(lv, tot, tol, sc.I)
    assert_grad(rgb.grad, tot["feats"][0], "rgb", tol)
    assert_grad(attr.grad, tot["feats"][2], "attributes", tol)
    assert_grad(fb.tap, tot["tap"], "tap", tol)
    assert_grad(fb.abs_tap, tot["abs_tap"], "abs_tap", tol)
    assert float(lv["position"].grad.abs().max()) > 0 and float(lv["rotation"].grad.abs().max()) > 0


@pytest.mark.parametrize("times", [TIMES, [7], [0, 1, 2, 5, 9, 14, 20, 26, 29]], ids=["F6", "F1", "F9"])
def test_per_frame_orthographic_cameras_train_against_the_oracle(oracle_mod, scene, times):
    _sets_against_oracle(oracle_mod, scene, times, tv._cameras(len(times)), None, 0.01, f"ortho F={len(times)}", 100)


@pytest.mark.parametrize("per_frame_intr", [False, True], ids=["intr4", "intrF4"])
def test_pinhole_cameras_train_against_the_oracle(oracle_mod, scene, per_frame_intr):
    F = len(TIMES)
    _sets_against_oracle(oracle_mod, scene, TIMES, tv._cameras(F), tv._intr(F if per_frame_intr else None), tv.NEAREST_PINHOLE,
                         f"pinhole per_frame_intr={per_frame_intr}", 1000)


def test_render_dynamic_trains_under_pinhole_cameras_against_the_oracle(oracle_mod, scene):
    """plain records, 3 channels: render_dynamic(extr [F,4,4], intr [F,4], differentiable=True)"""
    sc, F = scene, len(TIMES)
    extr, intr = tv._cameras(F), tv._intr(F)
    fb = FrameBatch(F, N, W, H, 3, "cuda", want_abs=True)
    lv = _leaves(sc)
    rgb = sc.rgb.clone().requires_grad_(True)
    out = fb.render_dynamic(sc.clock, TIMES, _t(extr), rgb, bg=1.0, nearest=tv.NEAREST_PINHOLE, intr=_t(intr), cubic_layout=0,
                            differentiable=True, **lv)
    g, = _image_grads(F, (3,), 77)
    out.backward(_t(g))
    torch.cuda.synchronize()
    fb.check()
    per, tot = occ.dynamic_frames_cam(oracle_mod, sc.clock, TIMES, sc.host, extr, intr, W, H,
                                      [dict(feature=sc.rgb_np, bg=1.0, taps=True)], [g], 0, tv.NEAREST_PINHOLE)
    pairs = fb.pairs.cpu().tolist()
    got = out.detach().cpu().numpy()
    for f, r in enumerate(per):
        assert pairs[f] > 1000, (f, pairs[f])
        np.testing.assert_allclose(fb.uv[f].cpu().numpy(), r["uv"], rtol=1e-5, atol=2e-4)
        bad = float((np.abs(got[f] - r["imgs"][0]) > (IMG_ATOL + IMG_RTOL * np.abs(r["imgs"][0]))).mean())
        assert bad < 1e-3, (f, bad)
    tol = GRAD_RTOL if _same_geometry(fb, per) else 5e-3
    _check_param_grads(lv, tot, tol, sc.I)
    assert_grad(rgb.grad, tot["feats"][0], "rgb", tol)
    assert_grad(fb.tap, tot["tap"], "tap", tol)
    assert_grad(fb.abs_tap, tot["abs_tap"], "abs_tap", tol)


# ------------------------------------------------------------------ 2. against the one-camera path
def _full_run(sc, extr, ordered, seed=5):
    """everything the one-camera path takes, under ``extr`` ([4,4] or [F,4,4]): outputs and every gradient"""
    F = len(TIMES)
    rng = np.random.default_rng(seed)
    fb = FrameBatch(F, N, W, H, 9, "cuda", want_abs=True)
    lv = _leaves(sc)
    lv["position"] = sc.model["position"].clone()                       # its gradient goes to the sink
    rgb, attr = sc.rgb.clone().requires_grad_(True), sc.attr.clone().requires_grad_(True)
    track = _t(rng.uniform(-1, 1, size=(F, N, 3)))                       # per frame; its gradient goes to the sink
    wide = _t(rng.uniform(-1, 1, size=(N, 40))).requires_grad_(True)
    pfeat = _t(rng.uniform(-1, 1, size=(N, 3))).requires_grad_(True)
    counts = [40, 0, 25, 40, 1, 40]
    xy = np.stack([rng.uniform(0, W - 1, size=sum(counts)), rng.uniform(0, H - 1, size=sum(counts))], 1)
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device="cuda")
    sink = {"position": torch.zeros_like(lv["position"]), "feature:2": torch.zeros_like(track)}
    sets = [dict(feature=rgb, bg=1.0, taps=True), dict(feature="depth", bg=1.0),
            dict(feature=[attr, track], bg=0.0, detach_opacity=True)]
    res = fb.render_dynamic_sets(sc.clock, TIMES, extr, sets, K=K, cubic_layout=0, differentiable=True, grad_sink=sink,
                                 wide=dict(feature=wide, bg=0.0, detach_opacity=True),
                                 points=dict(feature=pfeat, points=_t(xy), offsets=off, bg=0.0, detach_opacity=True, ordered=ordered),
                                 **lv)
    assert len(res) == 6                                                 # rgb depth attributes | wide | sparse | ids
    g = _image_grads(F, (3, 1, 5, 40), 9) + [np.random.default_rng(10).normal(size=(sum(counts), 3)).astype(np.float32)]
    torch.autograd.backward(list(res[:5]), [_t(x) for x in g])
    torch.cuda.synchronize()
    fb.check()
    grads = {k: lv[k].grad for k in TRAIN if k != "position"}
    grads.update(position=sink["position"], track=sink["feature:2"], rgb=rgb.grad, attr=attr.grad, wide=wide.grad, points=pfeat.grad,
                 tap=fb.tap.clone(), abs_tap=fb.abs_tap.clone())
    return [t.detach() for t in res[:5]], grads


@pytest.mark.parametrize("ordered", [False, True], ids=["points_atomic", "points_ordered"])
def test_equal_camera_copies_against_the_one_camera_path(scene, ordered):
    F = len(TIMES)
    e = _t(tv._cameras(3)[2])
    out1, g1 = _full_run(scene, e, ordered)
    outF, gF = _full_run(scene, e[None].repeat(F, 1, 1).contiguous(), ordered)
    for name, a, b in zip(("rgb", "depth", "attributes", "wide", "sparse"), outF, out1):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        bad = float((np.abs(a - b) > (IMG_ATOL + IMG_RTOL * np.abs(b))).mean())
        assert bad < 1e-3, (name, bad)
    assert sorted(g1) == sorted(gF)
    for k in g1:
        assert float(g1[k].abs().max()) > 0, k
        assert_grad(gF[k], g1[k].cpu().numpy(), k, GRAD_RTOL)


# ------------------------------------------------------------------ 3. the contract
def _simple(sc, fb, extr, intr=None, points=None, differentiable=True, nearest=0.01, seed=3):
    lv = _leaves(sc)
    rgb = sc.rgb.clone().requires_grad_(True)
    sets = [dict(feature=rgb, bg=1.0, taps=True), dict(feature="depth", bg=1.0), dict(feature=sc.attr, bg=0.0, detach_opacity=True)]
    kw = dict(differentiable=True) if differentiable else {}
    res = fb.render_dynamic_sets(sc.clock, TIMES, extr, sets, K=K, cubic_layout=0, intr=intr, nearest=nearest, points=points,
                                 **kw, **lv)
    outs = [t for t in res[:-1]]
    g = [_t(x) for x in _image_grads(len(TIMES), (3, 1, 2), seed)]
    if points is not None:
        g.append(torch.ones_like(outs[-1]))
    return res, lv, rgb, outs, g


def _grads_of(lv, rgb, fb):
    return {**{k: lv[k].grad.clone() for k in TRAIN}, "rgb": rgb.grad.clone(), "tap": fb.tap.clone()}


def test_one_camera_with_the_flag_is_the_default_path_bit_for_bit(scene):
    F = len(TIMES)
    e = _t(tv._cameras(3)[1])
    runs = []
    for flag in (False, True):
        fb = FrameBatch(F, N, W, H, 6, "cuda")
        res, lv, rgb, outs, g = _simple(scene, fb, e, differentiable=flag)
        torch.autograd.backward(outs, g)
        torch.cuda.synchronize()
        runs.append(([t.detach().clone() for t in res], _grads_of(lv, rgb, fb)))
    for a, b in zip(*[r[0] for r in runs]):
        assert torch.equal(a, b)
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_cameras_are_constants_and_the_default_still_refuses(scene):
    F = len(TIMES)
    fb = FrameBatch(F, N, W, H, 6, "cuda")
    extr = _t(tv._cameras(F))
    with pytest.raises(ValueError, match="cameras are constants"):
        _simple(scene, fb, extr.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="cameras are constants"):
        _simple(scene, fb, extr, intr=_t(tv._intr()).requires_grad_(True), nearest=tv.NEAREST_PINHOLE)
    with pytest.raises(ValueError, match="cameras are constants"):
        fb3 = FrameBatch(F, N, W, H, 3, "cuda")
        fb3.render_dynamic(scene.clock, TIMES, extr.clone().requires_grad_(True), scene.rgb, cubic_layout=0, differentiable=True,
                           **_leaves(scene))
    with pytest.raises(ValueError, match="forward only"):
        _simple(scene, fb, extr, differentiable=False)


def test_two_backward_passes_give_the_same_bits(scene):
    F = len(TIMES)
    extr, intr = _t(tv._cameras(F)), _t(tv._intr(F))
    for k_, nearest in ((None, 0.01), (intr, tv.NEAREST_PINHOLE)):
        runs = []
        for _ in range(2):
            fb = FrameBatch(F, N, W, H, 6, "cuda")
            res, lv, rgb, outs, g = _simple(scene, fb, extr, intr=k_, nearest=nearest)
            torch.autograd.backward(outs, g)
            torch.cuda.synchronize()
            runs.append(_grads_of(lv, rgb, fb))
        for k in runs[0]:
            assert torch.equal(runs[0][k], runs[1][k]), k
            assert float(runs[0][k].abs().max()) > 0, k


def test_deterministic_mode_takes_ordered_points_only(scene):
    F = len(TIMES)
    extr = _t(tv._cameras(F))
    rng = np.random.default_rng(12)
    counts = [8] * F
    xy = _t(np.stack([rng.integers(0, W, size=sum(counts)), rng.integers(0, H, size=sum(counts))], 1))
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device="cuda")
    pts = lambda ordered: dict(feature=scene.attr, points=xy, offsets=off, bg=0.0, detach_opacity=True, ordered=ordered)
    fb = FrameBatch(F, N, W, H, 6, "cuda")
    L.set_deterministic(True)
    try:
        res, lv, rgb, outs, g = _simple(scene, fb, extr, points=pts(False))
        with pytest.raises(L.SplatError, match="deterministic"):
            torch.autograd.backward(outs, g)
        runs = []
        for _ in range(2):
            res, lv, rgb, outs, g = _simple(scene, fb, extr, points=pts(True))
            torch.autograd.backward(outs, g)
            torch.cuda.synchronize()
            runs.append(_grads_of(lv, rgb, fb))
    finally:
        L.set_deterministic(False)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert float(runs[0]["position"].abs().max()) > 0
