"""The narrow forward (rows of at most four channels) fetches a 4x4 quarter's survivor list 16 entries at a time and hands
each survivor's operands to the quarter's 16 lanes by a DPP row broadcast; the wave leaves a chunk after the common count of
its four lists, rounded up to two.  This file drives that logic at its edges: scenes whose quarter lists have EVERY length
0 .. 35 (so 0, 1, 2, 15, 16, 17, 31, 32, 33: chunk boundaries, odd and even tails), one quarter long beside three empty ones,
whole waves without a survivor -- for C = 1 .. 4, with and without the id lists of the enhanced variant, single frame through
gs.alpha_blending* and as a FrameBatch.

The scene is built so that the lists can be COUNTED on the CPU from the oracle's tile lists and the cull rule (tile_cull:
bounding box of the alpha >= 1/255 ellipse against a quarter's rectangle of pixel centres): every splat is far smaller than
a quarter and sits near its quarter's centre, so the box keeps it on that quarter alone and no later stage of the cull can
drop it there.  The generator asserts that the lengths really occur.

Compared with the oracle as tests/test_gpu_parity.py does (images atol 1e-5 + rtol 1e-4, gradients through its assert_grad
with its defaults), ncontrib / gs_idx exactly; batch and per-frame images bit-equal as in tests/test_gpu_frames.py."""
import numpy as np
import pytest
import torch

from splatter_a_video_amd.synth import make_scene
from test_gpu_parity import IMG_ATOL, IMG_RTOL, assert_grad, dev, oracle_geometry

pytestmark = pytest.mark.gpu

W, H = 192, 128          # 12 x 8 tiles
SB = 128                 # the forward's super-batch: a tile list no longer than this is one set of quarter lists
NAMED = (0, 1, 2, 15, 16, 17, 31, 32, 33)
# list lengths of the four quarters of ONE wave of a tile (the tile's other three waves stay empty); together: every
# length 0 .. 35, long lists beside short and empty ones, a chunk that is exactly full (16, 32) and one entry over / under
PLAN = [(35, 0, 1, 2), (34, 3, 4, 5), (33, 6, 7, 8), (32, 9, 10, 11), (31, 12, 13, 14), (30, 15, 16, 17), (29, 18, 19, 20),
        (28, 21, 22, 23), (27, 24, 25, 26), (33, 0, 0, 0), (0, 0, 0, 16), (15, 0, 31, 0), (0, 32, 0, 0), (17, 0, 0, 0),
        (1, 0, 0, 0), (0, 0, 2, 0), (0, 35, 0, 0), (16, 16, 16, 16)]


def _pixel_to_world(o, sc):
    """the ortho camera's pixel coordinates are affine in x and in y: the map, from two probe points"""
    probe = np.array([[-0.5, -0.5, 0.5], [0.5, 0.5, 0.5]], np.float32)
    uv, _ = o.project_point_ortho_forward(probe, sc.extr, W, H, 0.01)
    ax, ay = (uv[1, 0] - uv[0, 0]), (uv[1, 1] - uv[0, 1])          # pixels per world unit
    bx, by = uv[0, 0] + 0.5 * ax, uv[0, 1] + 0.5 * ay              # pixel of world 0
    return lambda u, v: ((u - bx) / ax, (v - by) / ay)


def _scene(o, seed):
    rng = np.random.default_rng(seed)
    sc = make_scene(1, W, H, seed=seed)
    to_world = _pixel_to_world(o, sc)
    # one plan entry per tile, on tiles with even coordinates: no two of them touch, so what the binning adds to a neighbouring
    # tile's list (a splat's 3-sigma square may cross the tile's edge) lands in a tile that is otherwise empty
    tiles = rng.permutation((W // 32) * (H // 32))[:len(PLAN)]
    us, vs = [], []
    for k, (tile, lens) in enumerate(zip(tiles, PLAN)):
        tx, ty, w = 2 * (int(tile) % (W // 32)), 2 * (int(tile) // (W // 32)), k % 4
        for q, n in enumerate(lens):
            # centre of the quarter's 4 x 4 pixel centres, +- 0.3 px
            cx = 16 * tx + 8 * (w & 1) + 4 * (q & 1) + 1.5
            cy = 16 * ty + 8 * (w >> 1) + 4 * (q >> 1) + 1.5
            us.append(cx + rng.uniform(-0.3, 0.3, size=n)); vs.append(cy + rng.uniform(-0.3, 0.3, size=n))
    u, v = np.concatenate(us), np.concatenate(vs)
    N = u.size
    x, y = to_world(u, v)
    sc.N = N
    sc.xyz = np.stack([x, y, rng.permutation(N) / float(N) * 0.8 + 0.1], 1).astype(np.float32)   # distinct depths
    sc.phase = np.zeros(N, np.float32)
    # 0.1 .. 0.25 px along the three axes (the low-pass of the projection makes the footprint 0.6 px), each axis different
    # and randomly rotated: isotropic splats would leave the rotation gradient pure rounding noise
    axes = np.array([0.1, 0.17, 0.25]) * 2.0 / W
    sc.scale = np.stack([rng.permutation(axes) for _ in range(N)]).astype(np.float32)
    q = rng.normal(size=(N, 4))
    sc.rotate = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sc.opacity = rng.uniform(0.05, 0.6, size=(N, 1)).astype(np.float32)
    return sc


def _quarter_lengths(G, opacity):
    """lengths of the quarter lists [tile, wave, quarter] of the first super-batch under the cull's bounding-box rule; asserts that
    the rule's outcome is far from its thresholds and that a kept splat's centre lies inside the quarter (where neither the
    tangent-plane test nor an exact test can drop it)"""
    T = G["tr"].shape[0]
    lens = np.zeros((T, 4, 4), np.int64)
    for t in range(T):
        b, e = int(G["tr"][t, 0]), int(G["tr"][t, 1])
        assert e - b <= SB, "a tile list longer than one super-batch: the lists would not be the planned ones"
        tx0, ty0 = 16.0 * (t % (W // 16)), 16.0 * (t // (W // 16))
        for i in G["idx"][b:e]:
            (u, v), (ca, cb, cc), op = G["uv"][i].astype(np.float64), G["conic"][i].astype(np.float64), float(opacity[i, 0])
            assert 255.0 * op > 2.0
            tau = 2.0 * np.log(255.0 * op) * 1.002 + 2e-3
            det = ca * cc - cb * cb
            hx, hy = np.sqrt(tau * cc / det) * 1.001 + 0.01, np.sqrt(tau * ca / det) * 1.001 + 0.01
            for w in range(4):
                for q in range(4):
                    x0, y0 = tx0 + 8 * (w & 1) + 4 * (q & 1), ty0 + 8 * (w >> 1) + 4 * (q >> 1)
                    ax, ay = max(x0 - u, u - (x0 + 3.0), 0.0), max(y0 - v, v - (y0 + 3.0), 0.0)
                    assert abs(ax - hx) > 0.05 and abs(ay - hy) > 0.05, "box test too close to its threshold to be counted here"
                    if ax <= hx and ay <= hy:
                        assert ax == 0.0 and ay == 0.0, "a splat reaches a quarter it does not lie in"
                        lens[t, w, q] += 1
    return lens


def _checked_scene(o, seed):
    sc = _scene(o, seed)
    G = oracle_geometry(o, sc)
    assert G["vis"].all()
    lens = _quarter_lengths(G, sc.opacity)
    have = set(int(x) for x in lens.reshape(-1))
    assert set(range(36)) <= have, sorted(set(range(36)) - have)
    assert set(NAMED) <= have
    waves = lens.reshape(-1, 4)
    assert any(sorted(wv)[3] >= 32 and sorted(wv)[2] == 0 for wv in waves), "no long quarter beside three empty ones"
    assert any(wv.sum() == 0 for wv in waves) and any((wv == 16).all() for wv in waves)
    assert sorted(tuple(wv) for wv in waves if wv.sum()) == sorted(PLAN)
    return sc, G


@pytest.mark.parametrize("variant", ["plain", "enh"])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_every_list_length_single_frame(gpu, oracle_mod, C, variant):
    import dptr.gs as gs
    o = oracle_mod
    sc, G = _checked_scene(o, 100 + C)
    N, K, bg = sc.N, 6, 0.3
    rng = np.random.default_rng(C)
    feat = rng.uniform(size=(N, C)).astype(np.float32)
    kw = dict(K=K, enable_truncation=False)
    out_r, fT_r, nc_r, gi_r = o.alpha_blending_forward(G["uv"], G["conic"], sc.opacity, feat, G["idx"], G["tr"], bg, W, H, **kw)
    t = {k: dev(v, gpu).requires_grad_(True) for k, v in dict(uv=G["uv"], conic=G["conic"], opacity=sc.opacity, feat=feat).items()}
    idx, tr = gs.sort_gaussian(dev(G["uv"], gpu), dev(G["depth"], gpu), W, H, dev(G["radius"], gpu), dev(G["tiles"], gpu))
    assert (idx.cpu().numpy() == G["idx"]).all() and (tr.cpu().numpy() == G["tr"]).all()
    ndc = torch.zeros(N, 2, device=gpu, requires_grad=True)
    andc = torch.zeros(N, 2, device=gpu, requires_grad=True)
    if variant == "enh":
        out, nc, gi = gs.alpha_blending_enhanced(t["uv"], t["conic"], t["opacity"], t["feat"], idx, tr, bg, W, H, ndc, andc, **kw)
        assert (nc.cpu().numpy() == nc_r).all()
        assert (gi.cpu().numpy() == gi_r).all()
    else:
        out = gs.alpha_blending(t["uv"], t["conic"], t["opacity"], t["feat"], idx, tr, bg, W, H, ndc, andc)
    assert out.shape == (C, H, W)
    np.testing.assert_allclose(out.detach().cpu().numpy(), out_r, rtol=IMG_RTOL, atol=IMG_ATOL)
    g = rng.normal(size=(C, H, W)).astype(np.float32)
    (out * dev(g, gpu)).sum().backward()
    gr = o.alpha_blending_backward(G["uv"], G["conic"], sc.opacity, feat, G["idx"], G["tr"], bg, W, H, fT_r, nc_r, g)
    assert_grad(t["uv"].grad, gr[0], "dL_duv")
    assert_grad(t["conic"].grad, gr[1], "dL_dconic")
    assert_grad(t["opacity"].grad, gr[2], "dL_dopacity")
    assert_grad(t["feat"].grad, gr[3], "dL_dfeature")
    half = np.array([[0.5 * W, 0.5 * H]], np.float32)
    assert_grad(ndc.grad, gr[0] * half, "dL_dndc")
    assert_grad(andc.grad, gr[4] * half, "dL_dabs_ndc")


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_every_list_length_frame_batch(gpu, oracle_mod, C):
    """frame 0: the counted scene; frame 1: the same splats one quarter (4 px) to the right -- other lists, other tiles.  The batch
    renders both in one launch; images bit-equal to the per-frame operators, frame 0 within the image tolerance of the oracle."""
    import dptr.gs as gs
    from splatter_a_video_amd.frames import FrameBatch
    o = oracle_mod
    sc, G = _checked_scene(o, 200 + C)
    N, F, bg = sc.N, 2, 0.3
    rng = np.random.default_rng(10 + C)
    featv = rng.uniform(size=(N, C)).astype(np.float32)
    dx = _pixel_to_world(o, sc)(4.0, 0.0)[0] - _pixel_to_world(o, sc)(0.0, 0.0)[0]
    offv = np.zeros((F, N, 3), np.float32)
    offv[1, :, 0] = dx
    g = dev(rng.normal(size=(F, C, H, W)).astype(np.float32), gpu)
    off, extr = dev(offv, gpu), dev(sc.extr, gpu)

    def params():
        return {k: dev(v, gpu).requires_grad_(True) for k, v in dict(xyz=sc.xyz, scales=sc.scale, uquats=sc.rotate, opacity=sc.opacity,
                                                                     feat=featv).items()}

    pa = params()
    imgs = []
    for f in range(F):
        uv, depth, conic, radius, tiles = gs.preprocess_ortho(pa["xyz"], pa["scales"], pa["uquats"], extr, W, H, nearest=0.01, offset=off[f])
        idx, tr = gs.sort_gaussian(uv, depth, W, H, radius, tiles)
        img = gs.alpha_blending(uv, conic, pa["opacity"], pa["feat"], idx, tr, bg, W, H)
        (img * g[f]).sum().backward()
        imgs.append(img.detach())
    ref = torch.stack(imgs)

    pb = params()
    B = FrameBatch(F, N, W, H, C, "cuda")
    out = B.render(pb["xyz"], pb["scales"], pb["uquats"], pb["opacity"], pb["feat"], off, extr, bg=bg)
    assert out.shape == (F, C, H, W)
    assert torch.equal(out, ref)
    out.backward(g)
    torch.cuda.synchronize()
    assert B.check() > 0

    feat_r = featv
    out_r = o.alpha_blending_forward(G["uv"], G["conic"], sc.opacity, feat_r, G["idx"], G["tr"], bg, W, H)[0]
    np.testing.assert_allclose(out[0].detach().cpu().numpy(), out_r, rtol=IMG_RTOL, atol=IMG_ATOL)
    # same arithmetic per pair record, other summation order over the frames (tests/test_gpu_frames.py: close())
    for k in pa:
        a, b = pb[k].grad, pa[k].grad
        d = (a - b).abs()
        bad = d > 2e-4 * b.abs() + 2e-6 * float(b.abs().max()) + 1e-12
        assert int(bad.sum()) <= max(2, a.numel() // 100000), (k, int(bad.sum()))
        assert bool((d <= 2e-3 * b.abs() + 2e-5 * float(b.abs().max()) + 1e-12).all()), k
