"""Feature lifting under per-frame and pinhole cameras on the GPU (lift.FeatureLift.add / gradient / refine with extr= / intr=,
through splat_frame_preprocess_layer_batch_cam) against the project's dense route under the same cameras:
``FrameBatch.render_dynamic_sets(..., extr [F,4,4], intr=, wide=dict(feature=zeros [N, D + 1]), differentiable=True)`` with the
image gradient ``maps | ones`` -- the gradient with respect to the wide feature IS ``num`` (columns 0 .. D - 1) and ``den`` (column
D).  Bound 1 of tests/test_gpu_lift.py.  The small dynamic model of that file (300 Gaussians at 64 x 48, three frame times); the
cameras are those of tests/test_gpu_views.py moved two units back, so that the pinhole camera (nearest 0.2) sees the model whose
z lies in 0.1 .. 1."""
import numpy as np
import pytest
import torch

from test_gpu_lift import DH, DN, DW, HIDDEN, TIMES, _assert_close, _clip_maps, _feature_lift, _model, _t
from test_gpu_views import NEAREST_PINHOLE, _cameras

pytestmark = pytest.mark.gpu

NT = len(TIMES)


def _cams(pinhole):
    """(extr [3,4,4], intr [3,4] or None, nearest): x, y in +-1 at depth 2.1 .. 3.3 under focal lengths of 70 / 55 pixels stay
    inside the 64 x 48 image"""
    e = _cameras(NT).copy()
    e[:, 2, 3] += 2.0
    if not pinhole:
        return _t(e), None, 0.01
    k = np.array([70.0, 55.0, DW / 2 + 0.75, DH / 2 - 0.5], np.float32)
    intr = np.stack([k * np.array([1 + 0.03 * np.sin(f), 1 - 0.02 * np.cos(f), 1.0, 1.0], np.float32) for f in range(NT)])
    return _t(e), _t(intr), NEAREST_PINHOLE


def _dense_wide(feature, extr, intr, nearest, differentiable):
    """the wide set [3, c, H, W] of the dense route under the cameras (background 0, detached opacity)"""
    from splatter_a_video_amd.frames import FrameBatch
    params, clock, _ = _model()
    fb = FrameBatch(NT, DN, DW, DH, 3, "cuda")
    sets = [dict(feature=torch.zeros(DN, 3, device="cuda"), bg=0.0, taps=True)]
    res = fb.render_dynamic_sets(clock, list(TIMES), extr, sets, intr=intr, nearest=nearest, cubic_layout=0,
                                 wide=dict(feature=feature, bg=0.0, detach_opacity=True), differentiable=differentiable, **params)
    fb.check()
    return res[1]


@pytest.mark.parametrize("pinhole", [False, True], ids=["ortho", "pinhole"])
@pytest.mark.parametrize("D", [3, 33])
def test_add_under_cameras_against_the_dense_route(gpu, D, pinhole):
    extr, intr, nearest = _cams(pinhole)
    maps = _clip_maps(D)
    lift = _feature_lift(D, frames_per_batch=2, nearest=nearest).add(TIMES, maps, extr=extr, intr=intr)
    assert lift.fb.pair_records is None
    f = torch.zeros(DN, D + 1, device="cuda", requires_grad=True)
    out = _dense_wide(f, extr, intr, nearest, True)
    y = torch.cat([maps, torch.ones(NT, 1, DH, DW, device="cuda")], 1)
    (out * y).sum().backward()
    assert int((lift.den > 0).sum()) > DN // 2 and (lift.den[:HIDDEN] == 0).all()
    _assert_close(lift.num, f.grad[:, :D], f"D={D} pinhole={pinhole} num")
    _assert_close(lift.den, f.grad[:, D], f"D={D} pinhole={pinhole} den")
    # the cameras matter: the default camera gives other sums
    plain = _feature_lift(D, frames_per_batch=2).add(TIMES, maps)
    assert not torch.equal(plain.den, lift.den)
    # two runs give the same bits; one batch of four frames (padded) too; the one-call form is that object
    again = _feature_lift(D, frames_per_batch=2, nearest=nearest).add(TIMES, maps, extr=extr, intr=intr)
    assert torch.equal(again.num, lift.num) and torch.equal(again.den, lift.den)
    four = _feature_lift(D, frames_per_batch=4, nearest=nearest).add(TIMES, maps, extr=extr, intr=intr)
    assert torch.equal(four.num, lift.num) and torch.equal(four.den, lift.den)
    from splatter_a_video_amd.lift import lift_features
    f2, w2 = lift_features(*_model()[:2], TIMES, extr, DW, DH, maps, intr=intr, frames_per_batch=2, nearest=nearest)
    assert torch.equal(f2, lift.result()[0]) and torch.equal(w2, lift.den)


def test_default_call_keeps_its_bits(gpu):
    """no cameras: the launches of the one orthographic camera; the same camera handed to the call dispatches to them"""
    import splatter_a_video_amd._lib as L
    from splatter_a_video_amd.dynamics import frame_table
    D = 33
    maps = _clip_maps(D)
    params, clock, extr = _model()
    one = _feature_lift(D, frames_per_batch=4).add(TIMES, maps)
    assert one.camera is None
    # the geometry rows are the core entry point's, straight through the binding
    lib = L.lib()
    times = tuple(float(t) for t in TIMES) + (float(TIMES[-1]),)
    tab = frame_table(clock, list(times), torch.device("cuda"))
    o = dict(uv=torch.empty(4, DN, 2, device="cuda"), depth=torch.empty(4, DN, 1, device="cuda"), conic=torch.empty(4, DN, 3, device="cuda"),
             radius=torch.empty(4, DN, dtype=torch.int32, device="cuda"), opa_t=torch.empty(DN, 1, device="cuda"))
    L.check(lib.splat_frame_preprocess_layer_batch(
        4, DN, DN, DN, 0, clock.interval_num, L.ptr(tab), L.ptr(None), L.ptr(params["position"]), L.ptr(params["pos_cubic_node"]), 0,
        L.ptr(params["rotation"]), L.ptr(params["rot_poly_feat"]), L.ptr(params["rot_fourier_feat"]), L.ptr(params["opacity"]),
        L.ptr(params["scaling"]), L.ptr(extr), DW, DH, 0.01, 1.3, L.ptr(None), L.ptr(None), 1.0, 0, L.ptr(o["uv"]), L.ptr(o["depth"]),
        L.ptr(o["conic"]), L.ptr(o["radius"]), L.ptr(o["opa_t"]), L.stream()))
    for k in ("uv", "depth", "conic", "radius"):
        assert torch.equal(getattr(one.fb, k), o[k]), k
    assert torch.equal(one.opa_t, o["opa_t"])
    same = _feature_lift(D, frames_per_batch=4).add(TIMES, maps, extr=extr)
    assert torch.equal(same.num, one.num) and torch.equal(same.den, one.den)
    assert float(one.num.abs().max()) > 0


@pytest.mark.parametrize("pinhole", [False, True], ids=["ortho", "pinhole"])
def test_refine_under_cameras(gpu, pinhole):
    """the shape of tests/test_gpu_lift.py::test_refine with the cameras added: maps rendered from a hidden feature under the
    cameras, the lifted start, one gradient against the dense autograd gradient, and the fit lowers the residual"""
    D = 5
    extr, intr, nearest = _cams(pinhole)
    gen = torch.Generator(device="cuda").manual_seed(13)
    f_star = torch.rand(DN, D, device="cuda", generator=gen) * 2.0 - 1.0
    with torch.no_grad():
        maps = _dense_wide(f_star, extr, intr, nearest, False).contiguous()
    assert float(maps.abs().max()) > 0.1
    cams = dict(extr=extr, intr=intr)
    lift = _feature_lift(D, frames_per_batch=2, nearest=nearest).add(TIMES, maps, **cams)
    start, _ = lift.result()
    f = start.clone().requires_grad_(True)
    loss_ref = 0.5 * ((_dense_wide(f, extr, intr, nearest, True) - maps) ** 2).sum()
    loss_ref.backward()
    grad, loss = lift.gradient(TIMES, maps, start, **cams)
    _assert_close(grad, f.grad, "refine gradient under cameras")
    assert abs(float(loss) - float(loss_ref.detach())) <= 1e-3 * float(loss_ref.detach())
    iters = 50
    fitted, history = lift.refine(TIMES, maps, start, iters, lr=0.01, **cams)
    assert history.is_cuda and history.shape == (iters,) and fitted.shape == (DN, D)
    assert torch.equal(history[:1], loss), "the first entry is the loss at the lifted start"
    final = float(lift.gradient(TIMES, maps, fitted, **cams)[1])
    print(f"loss at the lifted start {float(history[0]):.6e}, after {iters} iterations {final:.6e}")
    assert final < float(history[0])
    assert not torch.equal(fitted, start) and torch.equal(start, lift.result()[0]), "the start is not modified"
    # without the cameras the same maps fit worse: the cameras reach the geometry of every call
    other = float(lift.gradient(TIMES, maps, fitted)[1])
    assert other > final
