"""Call SEQUENCES on the pooled one-call route: gs.rasterization_ortho / gs.rasterization render through frames.frame_rasterization,
a pool of one-frame batches keyed by (device, P, W, H, C) whose pair buffers live across calls.  Every test here renders the same
inputs through that stateful route and through a stateless one -- the operator chain preprocess_* -> sort_gaussian ->
alpha_blending, which sizes its lists exactly on every call -- and asks for bit-equal images and, by the `_close` rule of
tests/test_gpu_frame_rasterization.py, equal gradients.  Where the pair count GROWS between two calls of one key (grown scales,
another camera) the image is also compared with the CPU oracle's chain, an answer from outside the project's GPU code.

Scenes: make_scene(1500, 100, 60, seed=11), scales multiplied by 1 / 2 / 4 (28 tiles, partial tiles in both directions).  CPU
oracle, frame 0: the full lists hold 5119 (orthographic) / 6122 (pinhole) pairs at x1 and 20580 / 24943 at x4; in float64 3655 /
4390 resp. 13269 / 17752 of them have a pixel centre with alpha >= 1/255 in their tile, which any conservative reach mask must
keep.  A first call at x1 therefore reserves at most 5119 * 1.25 + 1024 = 7422 / 8676 entries and the x4 call cannot fit; each
test still asserts that from the batch itself (`check() > cap1`).

Inside a stream capture (torch.cuda.graph) the route neither synchronises nor resizes: the capacity is what the warm-up calls
reserved, and a replay whose frame outgrows it drops the surplus pairs and is reported by `frame_rasterization.last.check()`
after the replay.  tests/test_gpu_frame_rasterization.py::test_a_frame_loop_is_captured_in_a_hip_graph_and_replays_bit_equal pins
the capture itself."""
import numpy as np
import pytest
import torch

import dptr.gs as gs
from splatter_a_video_amd import frames as FR
from splatter_a_video_amd._lib import SplatError
from splatter_a_video_amd.gs import raster_ops as RO
from splatter_a_video_amd.synth import make_scene
from test_gpu_parity import IMG_ATOL, IMG_RTOL, oracle_geometry

pytestmark = pytest.mark.gpu

N, W, H, BG = 1500, 100, 60, 0.3
NAMES = ("xyz", "scale", "rotate", "opacity", "feature")


@pytest.fixture(autouse=True)
def _fresh_pool():
    """every test sizes its first batch itself: the pool of another test (or module) must not have grown the key already"""
    FR._FRAME_POOL.clear()
    yield
    FR._FRAME_POOL.clear()


def _t(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a), device="cuda", requires_grad=grad)


def _close(a, b, what):
    tol = 2e-4 * b.abs() + 2e-6 * float(b.abs().max()) + 1e-12
    assert bool(((a - b).abs() <= tol).all()), (what, float((a - b).abs().max()))


_SCENES = {}


def _scene(ortho, k=1.0, dz=0.0, C=3, P=N):
    """the scene at scale x k under the camera moved by dz along its view axis; frame 0's positions, the first P Gaussians"""
    key = (ortho, k, dz, C, P)
    if key not in _SCENES:
        sc = make_scene(N, W, H, seed=11, ortho=ortho)
        sc.scale = (sc.scale * np.float32(k)).astype(np.float32)
        sc.extr = sc.extr.copy()
        sc.extr[2, 3] += dz
        feat = np.random.default_rng(C).uniform(size=(N, C)).astype(np.float32)
        arrays = dict(xyz=sc.positions(0)[:P], scale=sc.scale[:P], rotate=sc.rotate[:P], opacity=sc.opacity[:P], feature=feat[:P])
        _SCENES[key] = (sc, arrays)
    return _SCENES[key]


def _grad_image(C=3):
    return _t(np.random.default_rng(100 + C).normal(size=(C, H, W)).astype(np.float32))


def _params(arrays, grad=True):
    return {k: _t(v, grad) for k, v in arrays.items()}


def _pooled(sc, p):
    if sc.ortho:
        return gs.rasterization_ortho(p["xyz"], p["scale"], p["rotate"], p["opacity"], p["feature"], _t(sc.extr), W, H, BG)
    assert RO.OPTIONS["rasterization_one_call"]
    return gs.rasterization(p["xyz"], p["scale"], p["rotate"], p["opacity"], p["feature"], _t(sc.intr), _t(sc.extr), W, H, BG)


def _chain(sc, p):
    """the stateless route: lists sized exactly on every call"""
    if sc.ortho:
        uv, depth, conic, radius, tiles = gs.preprocess_ortho(p["xyz"], p["scale"], p["rotate"], _t(sc.extr), W, H, nearest=0.01)
        idx, tr = gs.sort_gaussian(uv, depth, W, H, radius, tiles)
        return gs.alpha_blending(uv, conic, p["opacity"], p["feature"], idx, tr, BG, W, H)
    RO.OPTIONS["rasterization_one_call"] = False
    try:
        return gs.rasterization(p["xyz"], p["scale"], p["rotate"], p["opacity"], p["feature"], _t(sc.intr), _t(sc.extr), W, H, BG)
    finally:
        RO.OPTIONS["rasterization_one_call"] = True


_CHAIN = {}


def _chain_result(ortho, k=1.0, dz=0.0, C=3, P=N, grads=True):
    """image (and gradients under `_grad_image`) of the operator chain, computed once per scene and left unchanged"""
    key = (ortho, k, dz, C, P)
    if key not in _CHAIN or (grads and _CHAIN[key][1] is None):
        sc, arrays = _scene(*key)
        p = _params(arrays, grads)
        with torch.set_grad_enabled(grads):
            img = _chain(sc, p)
        if grads:
            img.backward(_grad_image(C))
        _CHAIN[key] = (img.detach(), {n: p[n].grad for n in NAMES} if grads else None)
    return _CHAIN[key]


def _pooled_step(ortho, k=1.0, dz=0.0, C=3, names=NAMES, what=""):
    """forward + backward of the pooled route against the chain's; returns the batch that rendered"""
    sc, arrays = _scene(ortho, k, dz, C)
    ref_img, ref_grads = _chain_result(ortho, k, dz, C)
    p = _params(arrays)
    img = _pooled(sc, p)
    fb = FR.frame_rasterization.last
    img.backward(_grad_image(C))
    assert torch.equal(img.detach(), ref_img), (what, "image", float((img.detach() - ref_img).abs().max()))
    for n in names:
        _close(p[n].grad, ref_grads[n], (what, n))
    return fb, img.detach()


def _oracle_image(oracle_mod, ortho, k=1.0, dz=0.0):
    sc, arrays = _scene(ortho, k, dz)
    G = oracle_geometry(oracle_mod, sc)
    return oracle_mod.alpha_blending_forward(G["uv"], G["conic"], sc.opacity, arrays["feature"], G["idx"], G["tr"], BG, W, H)[0]


def _assert_oracle(img, ref, what):
    """tests/test_gpu_parity.py's rule for a chain that runs its own geometry (test_rasterization_chain_matches_oracle): IMG_ATOL +
    IMG_RTOL |ref| on all but 1e-3 of the elements (a radius tie or an alpha = 1/255 decision may move a handful); dropped pairs
    move whole tiles"""
    bad = np.abs(img.cpu().numpy() - ref) > (IMG_ATOL + IMG_RTOL * np.abs(ref))
    print(f"{what}: {int(bad.sum())} of {bad.size} elements beyond atol {IMG_ATOL:g} + rtol {IMG_RTOL:g}")
    assert bad.mean() < 1e-3, (what, float(bad.mean()))


def _grow_then_shrink(oracle_mod, ortho, first, second):
    """case 1 / 2: a call, a call of the same key with more pairs than the first reserved, the first again"""
    fb, _ = _pooled_step(ortho, **first, what="first call")
    cap1 = fb.capacity
    fb2, img2 = _pooled_step(ortho, **second, what="call with more pairs")
    assert fb2 is fb, "the key's one batch has had its backward: it is the one to reuse (and to regrow)"
    _assert_oracle(img2, _oracle_image(oracle_mod, ortho, **second), "call with more pairs vs the CPU oracle")
    assert fb.check() > cap1, "the second call must hold more pairs than the first one reserved, else this test proves nothing"
    fb3, _ = _pooled_step(ortho, **first, what="first scene again")
    assert fb3 is fb
    fb.check()
    torch.cuda.synchronize()          # (a flag on its way to the host has arrived now: a late error would surface in the next call)
    sc, arrays = _scene(ortho, **first)
    with torch.no_grad():
        img = _pooled(sc, _params(arrays, False))
    assert torch.equal(img, _chain_result(ortho, **first)[0])
    FR.frame_rasterization.last.check()


def test_pairs_grow_between_calls_orthographic(oracle_mod):
    """x1 then x4 through gs.rasterization_ortho, same (P, W, H, C = 3): the second image and all five gradients are the chain's,
    the image is the oracle's, a third call at x1 is again the chain's, and no call or check() raises afterwards"""
    _grow_then_shrink(oracle_mod, True, dict(k=1.0), dict(k=4.0))


def test_pairs_grow_between_calls_pinhole_scales(oracle_mod):
    """the same through gs.rasterization (pinhole camera)"""
    _grow_then_shrink(oracle_mod, False, dict(k=1.0), dict(k=4.0))


# The camera of the pinhole scene moved along its view axis (extr[2, 3] += dz), CPU oracle: from dz = +16 the splats are small --
# the full lists hold 2751 pairs, so a first call there reserves at most int(2751 * 1.25) + 1024 = 4462 entries -- and at dz = -0.5
# 4582 pairs (float64) have a pixel centre with alpha >= 1/255 in their tile (full lists: 6473).
DZ_FAR, DZ_NEAR = 16.0, -0.5


def test_pairs_grow_between_calls_pinhole_camera(oracle_mod):
    """another camera instead of other scales: the first call from far away (dz = +16), the second close up (dz = -0.5)"""
    _grow_then_shrink(oracle_mod, False, dict(dz=DZ_FAR), dict(dz=DZ_NEAR))


@pytest.mark.parametrize("ortho", [True, False])
def test_evaluation_loop_under_no_grad(ortho):
    """six calls of one key alternating x1 / x4 / x2 under torch.no_grad(): every image is the chain's"""
    cap1 = None
    with torch.no_grad():
        for i, k in enumerate((1.0, 4.0, 2.0, 1.0, 4.0, 2.0)):
            sc, arrays = _scene(ortho, k)
            img = _pooled(sc, _params(arrays, False))
            ref = _chain_result(ortho, k, grads=False)[0]
            assert torch.equal(img, ref), (i, k, float((img - ref).abs().max()))
            fb = FR.frame_rasterization.last
            if cap1 is None:
                cap1 = fb.capacity
            elif k == 4.0:
                assert int(fb.pairs.max().item()) > cap1, "the x4 call must outgrow what the x1 call reserved"
    FR.frame_rasterization.last.check()


def test_no_grad_call_between_a_forward_and_its_backward():
    """img1 with grad at x1, a no_grad call at x4 for the same key, then img1.backward(): the gradients are the chain's -- the no_grad
    call has neither taken nor resized the batch whose backward was pending"""
    sc, arrays = _scene(True, 1.0)
    ref_img, ref_grads = _chain_result(True, 1.0)
    p = _params(arrays)
    img1 = _pooled(sc, p)
    fb1 = FR.frame_rasterization.last
    cap1, lists1 = fb1.capacity, fb1.idx_sorted
    sc4, arrays4 = _scene(True, 4.0)
    with torch.no_grad():
        img4 = _pooled(sc4, _params(arrays4, False))
    fb4 = FR.frame_rasterization.last
    assert torch.equal(img4, _chain_result(True, 4.0)[0])
    assert fb4 is not fb1 and fb4.check() > cap1          # (in fb1 the x4 frame would not have fitted)
    assert fb1.capacity == cap1 and fb1.idx_sorted is lists1
    img1.backward(_grad_image())
    assert torch.equal(img1.detach(), ref_img)
    for n in NAMES:
        _close(p[n].grad, ref_grads[n], n)


def test_more_live_forwards_than_the_pool_holds_per_key():
    """POOL_MAX + 1 grad-enabled forwards of one key before any backward: the POOL_MAX newest give the chain's gradients, the oldest
    one's batch was reused -- its backward raises the generation error instead of computing from another call's lists"""
    assert FR.POOL_MAX == 4
    sc, arrays = _scene(True, 1.0)
    ref_img, ref_grads = _chain_result(True, 1.0)
    g = _grad_image()
    live = []
    for _ in range(FR.POOL_MAX + 1):
        p = _params(arrays)
        live.append((p, _pooled(sc, p)))
    assert sum(len(v) for v in FR._FRAME_POOL.values()) == FR.POOL_MAX
    for p, img in live[1:]:
        img.backward(g)
        for n in NAMES:
            _close(p[n].grad, ref_grads[n], n)
    p, img = live[0]
    with pytest.raises(SplatError):
        img.backward(g)
    assert all(p[n].grad is None for n in NAMES)


def test_pairs_grow_between_calls_19_channels():
    """C = 19 (the wide kernel family behind the same pool), x1 -> x4: images, dL_dfeature, dL_dopacity"""
    fb, _ = _pooled_step(True, 1.0, C=19, names=("feature", "opacity"), what="x1")
    cap1 = fb.capacity
    fb2, _ = _pooled_step(True, 4.0, C=19, names=("feature", "opacity"), what="x4")
    assert fb2 is fb and fb.check() > cap1


def test_the_pool_is_bounded_over_all_shapes():
    """twelve Gaussian counts (a trainer that densifies: a new P every interval) under no_grad: every image is the chain's, the
    pool holds at most POOL_TOTAL batches over all keys, and clear_frame_pool() empties it"""
    sizes = list(range(1390, 1510, 10))          # the first P rows of the 1500-Gaussian scene
    assert len(sizes) == 12 and sizes[-1] == N and len(sizes) > FR.POOL_TOTAL
    with torch.no_grad():
        for P in sizes:
            sc, arrays = _scene(True, 1.0, P=P)
            img = _pooled(sc, _params(arrays, False))
            assert torch.equal(img, _chain_result(True, 1.0, P=P, grads=False)[0]), P
            assert sum(len(v) for v in FR._FRAME_POOL.values()) <= FR.POOL_TOTAL
    batches = [b for v in FR._FRAME_POOL.values() for b in v]
    assert 1 <= len(batches) <= FR.POOL_TOTAL
    assert [k[1] for k in FR._FRAME_POOL] == sizes[-len(batches):]          # least recently used first, the oldest keys gone
    assert sum(b.memory_bytes() for b in batches) <= FR.POOL_TOTAL * max(b.memory_bytes() for b in batches)
    FR.clear_frame_pool()
    assert not FR._FRAME_POOL
    with torch.no_grad():
        sc, arrays = _scene(True, 1.0)
        assert torch.equal(_pooled(sc, _params(arrays, False)), _chain_result(True, 1.0, grads=False)[0])
    assert sum(len(v) for v in FR._FRAME_POOL.values()) == 1


def test_the_bias_blend_refuses_reach_masked_lists(oracle_mod):
    """sort_gaussian_capped(conic=, opacity=) drops the pairs whose tile the splat cannot reach with opacity * G >= 1/255:
    alpha_blending composites the same image from them (the control), alpha_blending_with_bias -- whose alpha = opacity * G + bias
    reaches 1/255 in tiles that test dropped -- raises ValueError, and with the full lists it is the oracle's image"""
    o = oracle_mod
    sc, arrays = _scene(True, 1.0)
    G = oracle_geometry(o, sc)
    uv, depth, conic, radius, tiles = (_t(G[n]) for n in ("uv", "depth", "conic", "radius", "tiles"))
    opacity, feature = _t(arrays["opacity"]), _t(arrays["feature"])
    idx, tr = gs.sort_gaussian(uv, depth, W, H, radius, tiles)
    idx_r, tr_r, status = gs.sort_gaussian_capped(uv, depth, W, H, radius, None, conic, opacity)
    assert 0 < idx_r.numel() < idx.numel() and status.reach
    assert torch.equal(gs.alpha_blending(uv, conic, opacity, feature, idx_r, tr_r, BG, W, H),
                       gs.alpha_blending(uv, conic, opacity, feature, idx, tr, BG, W, H))
    bias = np.full((N, 1), 0.02, np.float32)
    with pytest.raises(ValueError):
        gs.alpha_blending_with_bias(uv, conic, opacity, feature, _t(bias), idx_r, tr_r, BG, W, H)
    out = gs.alpha_blending_with_bias(uv, conic, opacity, feature, _t(bias), idx, tr, BG, W, H)
    ref = o.alpha_blending_forward(G["uv"], G["conic"], sc.opacity, arrays["feature"], G["idx"], G["tr"], BG, W, H, opacity_bias=bias)[0]
    print("bias, full lists: worst", float(np.abs(out.cpu().numpy() - ref).max()))
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=IMG_RTOL, atol=IMG_ATOL)
