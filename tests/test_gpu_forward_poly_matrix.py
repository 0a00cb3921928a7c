"""The narrow forward (rows of at most four channels, no bias) takes the exponent polynomial of a quarter's survivors from the
matrix pipe: per group of four list entries six chained v_mfma_f32_4x4x1_16b_f32 (cbsz:2 abid:group) over the monomials
1 x y xx xy yy.  Rows of five channels and more evaluate the same polynomial with power_poly() on the VALU, in
the generic lane = pixel loop.  Both see the same lists, the same cull and the same compositing arithmetic, so the SAME scene
with zero-valued channels appended up to C = 5 must give, for channels 0 .. C-1, final_T, ncontrib and (enhanced variant)
gs_idx, exactly the bits of the narrow route: every pixel, no tolerance.  (cull_flags are not compared: the narrow route
publishes the applied (entry, quarter) pairs, the other a superset.)  The property holds for the VALU form of the narrow
forward as well: this file passes on the commit before the matrix form.

Scenes: a general one (100 x 60, 1500 rotated anisotropic Gaussians under a rotated camera, an opaque spot: the oracle
confirms on the CPU that most pixels have contributors and that some saturate) and one of hard operands (64 x 48: opacity 0
and 1e-30, centre alphas on both sides of 1/255, needle conics with coefficients above 1e4, splats exactly on pixel centres
and on the tile centre, a NaN conic and an infinite uv in the middle of the lists; the lists come from gs.sort_gaussian,
without conic / opacity, so that no reach mask drops those pairs before the kernel).  The backward (two v_mfma_f32_16x16x4_f32
per step for the same polynomial) must replay every decision of the new forward: T_front = 1 as in tests/test_gpu_frames.py."""
import functools

import numpy as np
import pytest
import torch

from splatter_a_video_amd.synth import make_scene
from test_gpu_parity import dev, oracle_geometry

pytestmark = pytest.mark.gpu

CW = 5   # the narrowest row that takes the generic loop (rows of up to four channels ride in the coefficient block)
VARIANTS = [("plain", 0, False), ("enh", 20, False), ("trunc", 2, True)]


def _rotated_camera():
    th = 0.3
    E = np.eye(4, dtype=np.float32)
    E[:3, :3] = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], np.float32) @ \
        np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]], np.float32)
    E[:3, 3] = np.array([0.05, -0.1, 0.3], np.float32)
    return E


@functools.lru_cache(maxsize=None)
def _general(o):
    """(scene, oracle geometry of frame 0): 100 x 60, 1500 Gaussians, rotated camera, an opaque spot of radius 8 px"""
    W, H, N = 100, 60, 1500
    sc = make_scene(N, W, H, seed=13, clustered=0.3, cluster_area=0.03, blobs=1)
    sc.extr = _rotated_camera()
    G = oracle_geometry(o, sc)
    uv = G["uv"]
    inside = (uv[:, 0] > 8) & (uv[:, 0] < W - 8) & (uv[:, 1] > 8) & (uv[:, 1] < H - 8)
    hist, xe, ye = np.histogram2d(uv[inside, 0], uv[inside, 1], bins=[W // 4, H // 4], range=[[0, W], [0, H]])
    bx, by = np.unravel_index(np.argmax(hist), hist.shape)
    sc.opacity[(uv[:, 0] - (xe[bx] + 2)) ** 2 + (uv[:, 1] - (ye[by] + 2)) ** 2 < 64] = np.float32(0.99)
    feat = np.random.default_rng(1).uniform(size=(N, 1)).astype(np.float32)
    _, fT, nc = o.alpha_blending_forward(uv, G["conic"], sc.opacity, feat, G["idx"], G["tr"], 0.0, W, H)
    assert (nc > 0).mean() > 0.5, "most pixels of the general scene must have a contributor"
    assert int((fT < 1e-3).sum()) >= 10, "some pixels of the general scene must saturate"
    a, b, c = G["conic"][G["vis"]].T
    assert (np.abs(b) > 0.05 * np.sqrt(a * c)).mean() > 0.5, "rotated anisotropic conics"
    return sc, G


@functools.lru_cache(maxsize=None)
def _hard(o):
    """64 x 48, 320 Gaussians; (W, H, N, uv for the sort, depth, radius, tiles, uv / conic / opacity for the blend)"""
    W, H, N = 64, 48, 320
    sc = make_scene(N, W, H, seed=5, sigma_px=3.0)
    G = oracle_geometry(o, sc)
    assert G["vis"].all()
    uv, conic, op = G["uv"].copy(), G["conic"].copy(), sc.opacity.copy()
    op[0:10] = 0.0
    op[10:20] = np.float32(1e-30)
    # centre alpha = opacity: on both sides of 1/255 and exactly on it, the splats on pixel centres so that the centre is evaluated
    edge = np.float32(1.0 / 255.0)
    op[20:60, 0] = np.array([edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1)), edge * np.float32(1 - 1e-4),
                             edge * np.float32(1 + 1e-4)] * 8, np.float32)
    uv[20:60] = np.floor(uv[20:60])
    # needle-thin conics: coefficients above 1e4 (the radius of the sort stays what it was: the pairs reach the kernel)
    ang = np.random.default_rng(6).uniform(0, np.pi, size=40)
    big, small = 3e4, 0.02
    cs, sn = np.cos(ang), np.sin(ang)
    conic[60:100] = np.stack([big * cs * cs + small * sn * sn, (big - small) * cs * sn, big * sn * sn + small * cs * cs], 1).astype(np.float32)
    assert float(np.abs(conic[60:100]).max()) > 1e4
    uv[60:80] = np.floor(uv[60:80])       # half of the needles through a pixel centre
    # exactly on pixel centres and on tile centres (7.5 + 16 k): zero linear terms of the polynomial
    uv[100:130] = np.floor(uv[100:130])
    uv[130:150] = np.floor(uv[130:150] / 16.0) * 16.0 + 7.5
    op[130:140] = 1.0                       # log2(o) = 0: the polynomial is exactly zero at the tile centre
    conic[150:155] = np.float32("nan")
    conic[155:158, 0] = np.float32("inf")
    uv[158:163, 0] = np.float32("inf")
    uv[163:166] = np.float32("nan")
    # in the middle of the lists: some tile holds such an entry neither first nor last
    mid = False
    for b, e in G["tr"]:
        ids = G["idx"][b:e]
        mid |= bool(e - b >= 3 and np.isin(ids[1:-1], np.arange(150, 166)).any())
    assert mid, "no NaN / inf entry in the middle of a tile list"
    return W, H, N, G, uv, conic, op


def _blend(gpu, W, H, sort_in, blend_in, feat, K, trunc, bg=0.3):
    """gs.alpha_blending* -> (image [C,H,W], final_T, ncontrib, gs_idx or None) with lists from gs.sort_gaussian"""
    import dptr.gs as gs
    uv_s, depth, radius, tiles = (dev(a, gpu) for a in sort_in)
    idx, tr = gs.sort_gaussian(uv_s, depth, W, H, radius, tiles)
    uv, conic, op = (dev(a, gpu) for a in blend_in)
    f = dev(feat, gpu).requires_grad_(True)   # (a graph node: the forward's final_T and ncontrib are what it saved for the backward)
    if K:
        out, nc, gi = gs.alpha_blending_enhanced(uv, conic, op, f, idx, tr, bg, W, H, K=K, enable_truncation=trunc)
    else:
        out, gi = gs.alpha_blending(uv, conic, op, f, idx, tr, bg, W, H), None
    saved = out.grad_fn.saved_tensors
    final_T, ncontrib = saved[6], saved[7]
    assert final_T.shape == (H, W) and ncontrib.dtype == torch.int32
    if K:
        assert torch.equal(nc, ncontrib)
    return out.detach(), final_T, ncontrib, gi


def _pad(feat):
    return np.concatenate([feat, np.zeros((feat.shape[0], CW - feat.shape[1]), np.float32)], 1)


def _same(narrow, wide, C):
    out_n, fT_n, nc_n, gi_n = narrow
    out_w, fT_w, nc_w, gi_w = wide
    # bit patterns, so that a NaN pixel (none is expected) or a zero of the other sign would count
    assert torch.equal(out_n.view(torch.int32), out_w[:C].view(torch.int32)), int((out_n != out_w[:C]).sum())
    assert torch.equal(fT_n.view(torch.int32), fT_w.view(torch.int32))
    assert torch.equal(nc_n, nc_w)
    if gi_n is not None:
        assert torch.equal(gi_n, gi_w)
    assert bool(torch.isfinite(out_n).all())


@pytest.mark.parametrize("variant,K,trunc", VARIANTS)
@pytest.mark.parametrize("C", [1, 3])
def test_general_scene_single_frame(gpu, oracle_mod, C, variant, K, trunc):
    sc, G = _general(oracle_mod)
    feat = np.random.default_rng(20 + C).uniform(size=(sc.N, C)).astype(np.float32)
    sort_in = (G["uv"], G["depth"], G["radius"], G["tiles"])
    blend_in = (G["uv"], G["conic"], sc.opacity)
    narrow = _blend(gpu, sc.W, sc.H, sort_in, blend_in, feat, K, trunc)
    wide = _blend(gpu, sc.W, sc.H, sort_in, blend_in, _pad(feat), K, trunc)
    _same(narrow, wide, C)
    # not vacuous on the GPU either (a pixel that truncation stops after K = 2 contributors does not get to saturate)
    assert float((narrow[2] > 0).float().mean()) > 0.5 and (trunc or int((narrow[1] < 1e-3).sum()) >= 10)
    if K:
        assert int((narrow[3] >= 0).sum()) > 0


@pytest.mark.parametrize("variant,K,trunc", VARIANTS)
@pytest.mark.parametrize("C", [1, 3])
def test_hard_operands_single_frame(gpu, oracle_mod, C, variant, K, trunc):
    W, H, N, G, uv, conic, op = _hard(oracle_mod)
    feat = np.random.default_rng(30 + C).uniform(size=(N, C)).astype(np.float32)
    sort_in = (G["uv"], G["depth"], G["radius"], G["tiles"])       # the clean geometry makes the lists
    narrow = _blend(gpu, W, H, sort_in, (uv, conic, op), feat, K, trunc)
    wide = _blend(gpu, W, H, sort_in, (uv, conic, op), _pad(feat), K, trunc)
    _same(narrow, wide, C)
    assert float((narrow[2] > 0).float().mean()) > 0.5


@pytest.mark.parametrize("variant,K", [("plain", 0), ("enh", 20)])
@pytest.mark.parametrize("C", [1, 3])
def test_general_scene_frame_batch(gpu, oracle_mod, C, variant, K):
    from splatter_a_video_amd.frames import FrameBatch
    sc, _ = _general(oracle_mod)
    N, W, H, F, bg = sc.N, sc.W, sc.H, 3, 0.3
    feat = np.random.default_rng(40 + C).uniform(size=(N, C)).astype(np.float32)
    off = dev(np.stack([sc.positions(f) - sc.xyz for f in range(F)]).astype(np.float32), gpu)
    geo = [dev(a, gpu) for a in (sc.xyz, sc.scale, sc.rotate, sc.opacity)]
    extr = dev(sc.extr, gpu)

    def run(fe):
        B = FrameBatch(F, N, W, H, fe.shape[1], "cuda")
        f = dev(fe, gpu)
        with torch.no_grad():
            if K:
                out, gi = B.render_sets(*geo, [dict(feature=f, bg=bg, taps=True)], off, extr, K=K)
            else:
                out, gi = B.render(*geo, f, off, extr, bg=bg), None
        torch.cuda.synchronize()
        B.check()
        return out, B.final_T.clone(), B.ncontrib.clone(), gi

    out_n, fT_n, nc_n, gi_n = run(feat)
    out_w, fT_w, nc_w, gi_w = run(_pad(feat))
    assert out_n.shape == (F, C, H, W)
    assert torch.equal(out_n.view(torch.int32), out_w[:, :C].view(torch.int32))
    assert torch.equal(fT_n.view(torch.int32), fT_w.view(torch.int32)) and torch.equal(nc_n, nc_w)
    if K:
        assert torch.equal(gi_n, gi_w)
    assert float((nc_n > 0).float().mean()) > 0.5 and int((fT_n < 1e-3).sum()) >= 10


@pytest.mark.parametrize("C", [1, 3])
def test_backward_replays_the_new_forward(gpu, oracle_mod, C):
    """the backward's 16x16x4 MFMA polynomial makes every decision of the forward's 4x4x1 one: the transmittance its back-to-front
    replay arrives at in front of the first splat is 1 on every pixel (tests/test_gpu_frames.py: < 2e-4)"""
    import dptr.gs as gs
    from splatter_a_video_amd.frames import FrameBatch
    from splatter_a_video_amd.gs.raster_ops import capture_T_front
    sc, G = _general(oracle_mod)
    N, W, H, F = sc.N, sc.W, sc.H, 3
    rng = np.random.default_rng(50 + C)
    feat = rng.uniform(size=(N, C)).astype(np.float32)
    t = {k: dev(v, gpu).requires_grad_(True) for k, v in dict(uv=G["uv"], conic=G["conic"], opacity=sc.opacity, feat=feat).items()}
    idx, tr = gs.sort_gaussian(dev(G["uv"], gpu), dev(G["depth"], gpu), W, H, dev(G["radius"], gpu), dev(G["tiles"], gpu))
    out = gs.alpha_blending(t["uv"], t["conic"], t["opacity"], t["feat"], idx, tr, 0.3, W, H)
    with capture_T_front() as cap:
        out.backward(dev(rng.normal(size=(C, H, W)).astype(np.float32), gpu))
    torch.cuda.synchronize()
    assert len(cap.maps) == 1 and float((cap.maps[0] - 1).abs().max()) < 2e-4
    assert float(t["conic"].grad.abs().max()) > 0

    p = {k: dev(v, gpu).requires_grad_(True) for k, v in dict(xyz=sc.xyz, scales=sc.scale, uquats=sc.rotate, opacity=sc.opacity, feat=feat).items()}
    off = dev(np.stack([sc.positions(f) - sc.xyz for f in range(F)]).astype(np.float32), gpu)
    B = FrameBatch(F, N, W, H, C, "cuda")
    img = B.render(p["xyz"], p["scales"], p["uquats"], p["opacity"], p["feat"], off, dev(sc.extr, gpu), bg=0.3)
    with capture_T_front() as cap:
        img.backward(dev(rng.normal(size=(F, C, H, W)).astype(np.float32), gpu))
    torch.cuda.synchronize()
    assert B.check() > 0
    assert float((cap.maps[0] - 1).abs().max()) < 2e-4
