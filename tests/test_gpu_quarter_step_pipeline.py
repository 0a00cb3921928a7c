"""The quarter-list backward of narrow rows (blend_bwd_quarter_kernel) walks, per 4x4 quarter of a wave's block, a survivor
list in steps of 16 entries; a step reads its entries, their operands and, in its epilogue, the slab rows it adds to.  This
file drives the shapes at which a change to the order of those reads inside and across steps can go wrong (a
software-pipelined step was built and measured; whatever order the kernel keeps, these are its edges):

  * quarter lists of every length 0 .. 35 in one wave beside empty quarters (a prefetch past a list's end, into the next
    non-empty list, into the pad), a quarter between an empty predecessor and an empty successor;
  * more than 80 survivors of one wave inside one 128-entry super-batch: a second round of the slab (p0 = CAP, records added
    to what the first round stored);
  * a tile list of more than 256 entries: three super-batches, the staging and the cull words rotate;
  * THE hazard: an entry that is the last of quarter G's list and the first of quarter G + 1's (a splat a few pixels wide on
    the middle of a wave's 8x8 block, everything else of quarter G behind it, everything else of quarter G + 1 in front) --
    two consecutive steps add to the same slab row, the second one's read must see the first one's write.

The scene is built like that of tests/test_gpu_blend_chunk_tails.py: tiny splats near the centre of their quarter, one plan
entry per tile on tiles that do not touch.  The lists are COUNTED on the CPU from the oracle's tile lists, its ncontrib and
alpha in float64 (a narrow row's list of a quarter = the entries that applied to one of its 16 pixels), every
decision far from its threshold, and the generator asserts that the lengths and coincidences above really occur; the frame
batch's own cull words must say the same.

C = 1 and 3, with and without the abs taps, as a single frame through gs.alpha_blending and as a two-frame FrameBatch (frame
1: the same splats 4 px to the right).  Against the oracle with tests/test_gpu_parity.py's tolerances (images atol 1e-5 + rtol
1e-4, gradients through assert_grad with its defaults); everything runs twice and must be bit-equal (the single-frame
operators in deterministic mode: their block-level backward otherwise adds carried survivors with float atomics)."""
import copy
import functools

import numpy as np
import pytest
import torch

from splatter_a_video_amd.synth import make_scene
from test_gpu_blend_chunk_tails import PLAN, _pixel_to_world
from test_gpu_parity import IMG_ATOL, IMG_RTOL, assert_grad, dev, oracle_geometry

pytestmark = pytest.mark.gpu

W, H = 192, 128          # 12 x 8 tiles
SB, CAP = 128, 80        # QuarterCfg: entries of a super-batch, slab rows of a wave and round
F = 2
BG = 0.3
SEED = 31
# per tile: ("tiny", [per wave: lengths of its four quarters]) | ("hazard", k): one wide splat on the middle of wave k % 4's
# block, k tiny splats BEHIND it in quarters 0 and 2, k in FRONT of it in quarters 1 and 3
EXTRA = [("tiny", [(30, 28, 25, 12), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]),         # 95 rows in one wave, one super-batch
         ("tiny", [(20, 18, 17, 16), (16, 20, 18, 17), (17, 16, 20, 18), (18, 17, 16, 20)]),   # 284 entries: three super-batches
         ("hazard", 0), ("hazard", 3), ("hazard", 15), ("hazard", 16)]


def _scene(o, seed=SEED):
    rng = np.random.default_rng(seed)
    sc = make_scene(1, W, H, seed=seed)
    to_world = _pixel_to_world(o, sc)
    plans = [("tiny", [lens if w == k % 4 else (0, 0, 0, 0) for w in range(4)]) for k, lens in enumerate(PLAN)] + EXTRA
    tiles = rng.permutation((W // 32) * (H // 32))[:len(plans)]      # tiles with even coordinates: no two of them touch
    assert len(plans) <= (W // 32) * (H // 32)
    u, v, z, wide = [], [], [], []

    def tiny(tx, ty, w, q, n, zlo, zhi):
        cx = 16 * tx + 8 * (w & 1) + 4 * (q & 1) + 1.5               # centre of the quarter's 4 x 4 pixel centres, +- 0.3 px
        cy = 16 * ty + 8 * (w >> 1) + 4 * (q >> 1) + 1.5
        u.extend(cx + rng.uniform(-0.3, 0.3, size=n)); v.extend(cy + rng.uniform(-0.3, 0.3, size=n))
        z.extend(rng.uniform(zlo, zhi, size=n)); wide.extend([False] * n)

    for k, (tile, (kind, spec)) in enumerate(zip(tiles, plans)):
        tx, ty = 2 * (int(tile) % (W // 32)), 2 * (int(tile) // (W // 32))
        if kind == "tiny":
            for w, lens in enumerate(spec):
                for q, n in enumerate(lens):
                    tiny(tx, ty, w, q, n, 0.1, 0.9)
        else:
            w = k % 4
            u.append(16 * tx + 8 * (w & 1) + 3.5); v.append(16 * ty + 8 * (w >> 1) + 3.5); z.append(0.5); wide.append(True)
            for q in range(4):
                tiny(tx, ty, w, q, spec, *((0.6, 0.9) if q in (0, 2) else (0.1, 0.4)))
    N = len(u)
    x, y = to_world(np.asarray(u), np.asarray(v))
    wide = np.asarray(wide)
    sc.N = N
    zr = np.empty(N)
    zr[np.argsort(np.asarray(z), kind="stable")] = np.arange(N) / float(N) * 0.8 + 0.1   # the drawn order, at distinct float32 depths
    sc.xyz = np.stack([x, y, zr], 1).astype(np.float32)
    assert np.unique(sc.xyz[:, 2]).size == N, "distinct depths"
    sc.phase = np.zeros(N, np.float32)
    # tiny: 0.1 .. 0.25 px along the three axes (the low-pass of the projection makes the footprint 0.6 px); wide: 0.8 .. 1.2 px --
    # each axis different and randomly rotated: isotropic splats would leave the rotation gradient pure rounding noise
    axes = np.array([0.1, 0.17, 0.25]) * 2.0 / W
    sc.scale = np.stack([rng.permutation(axes) * (4.8 if wd else 1.0) for wd in wide]).astype(np.float32)
    q = rng.normal(size=(N, 4))
    sc.rotate = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sc.opacity = np.where(wide, 0.5, rng.uniform(0.05, 0.6, size=N)).astype(np.float32).reshape(N, 1)
    return sc


def _lists(G, opacity, nc):
    """{tile: (n, applied[n, wave, quarter], [batch][wave][quarter] -> entries e of the super-batch, ascending = back to front)}:
    the quarter lists of the backward, counted from the oracle's tile lists.  Entry at list position p applied on a pixel iff
    alpha >= 1/255 there and p < ncontrib of the pixel; asserts that no quarter's decision hangs on an alpha within 10 % of 1/255."""
    out = {}
    gx = W // 16
    py, px = np.mgrid[0:16, 0:16].astype(np.float64)
    for t in range(G["tr"].shape[0]):
        b, e = int(G["tr"][t, 0]), int(G["tr"][t, 1])
        if e == b:
            continue
        ids = G["idx"][b:e]
        x0, y0 = 16 * (t % gx), 16 * (t // gx)
        ncT = nc[y0:y0 + 16, x0:x0 + 16].astype(np.int64)
        n = min(e - b, int(ncT.max()))
        if n == 0:
            continue
        uv, con, op = G["uv"][ids].astype(np.float64), G["conic"][ids].astype(np.float64), opacity[ids, 0].astype(np.float64)
        dx, dy = (x0 + px)[None] - uv[:, 0, None, None], (y0 + py)[None] - uv[:, 1, None, None]
        power = -0.5 * (con[:, 0, None, None] * dx * dx + con[:, 2, None, None] * dy * dy) - con[:, 1, None, None] * dx * dy
        alpha = op[:, None, None] * np.exp(power)
        live = np.arange(e - b)[:, None, None] < ncT[None]

        def quarters(m):     # [L, 16, 16] -> [L, wave, quarter]
            m = m.reshape(-1, 2, 2, 4, 2, 2, 4).any(axis=(3, 6))          # [L, wy, qy, wx, qx]
            return m.transpose(0, 1, 3, 2, 4).reshape(-1, 4, 4)           # wave = wx + 2 wy, quarter = qx + 2 qy
        hi, lo = quarters((alpha > 1.1 / 255.0) & live), quarters((alpha > 0.9 / 255.0) & live)
        assert (hi == lo).all(), f"tile {t}: a quarter's decision within 10 % of alpha = 1/255"
        app = hi[:n]
        batches = []
        for top in range(n - 1, -1, -SB):
            nb = min(SB, top + 1)
            batches.append([[[ee for ee in range(nb) if app[top - ee, w, q]] for q in range(4)] for w in range(4)])
        out[t] = (n, app, batches)
    return out


def _assert_shapes(lists):
    lens, hazard_full, hazard_one, hazard_mid = set(), 0, 0, 0
    second_round = three_batches = lonely = False
    for t, (n, app, batches) in lists.items():
        three_batches |= n > 2 * SB and len(batches) >= 3
        for wl in (wl for bt in batches for wl in bt):
            cq = [len(x) for x in wl]
            if sum(cq):
                lens.update(cq)
            second_round |= len(set().union(*wl)) > CAP and n <= SB
            lonely |= any(cq[g] and not cq[g - 1] and not cq[g + 1] for g in (1, 2))
            for g in range(3):
                if cq[g] and cq[g + 1] and wl[g][-1] == wl[g + 1][0]:      # the same slab row in two consecutive steps
                    hazard_one += cq[g] == 1 and cq[g + 1] == 1
                    hazard_full += cq[g] % 16 == 0 or cq[g + 1] > 16
                    hazard_mid += 1
    assert set(range(36)) <= lens, sorted(set(range(36)) - lens)
    assert lonely, "no quarter between an empty predecessor and an empty successor"
    assert second_round, "no wave with more than CAP survivors inside a one-batch tile"
    assert three_batches, "no tile list of three super-batches"
    assert hazard_one >= 2 and hazard_full >= 2 and hazard_mid >= 8, (hazard_one, hazard_full, hazard_mid)


@functools.lru_cache(maxsize=None)
def _reference(o):
    """scene, per frame the oracle's geometry, forward results per channel count and the counted lists: computed once"""
    sc = _scene(o)
    to_world = _pixel_to_world(o, sc)
    dxw = float(to_world(4.0, 0.0)[0] - to_world(0.0, 0.0)[0])
    frames = []
    for f in range(F):
        s2 = copy.copy(sc)
        s2.xyz = sc.xyz.copy()
        s2.xyz[:, 0] += np.float32(dxw * f)
        G = oracle_geometry(o, s2)
        assert G["vis"].all()
        frames.append(G)
    fwd = {}
    for C in (1, 3):
        feat = np.random.default_rng(C).uniform(size=(sc.N, C)).astype(np.float32)
        fwd[C] = (feat, [o.alpha_blending_forward(G["uv"], G["conic"], sc.opacity, feat, G["idx"], G["tr"], BG, W, H)[:3] for G in frames])
    lists = [_lists(G, sc.opacity, fwd[3][1][f][2]) for f, G in enumerate(frames)]
    _assert_shapes(lists[0])
    return dict(sc=sc, dxw=dxw, G=frames, fwd=fwd, lists=lists)


def _oracle_backward(o, R, C, f, g):
    sc, G = R["sc"], R["G"][f]
    feat, res = R["fwd"][C]
    _, fT, nc = res[f]
    return o.alpha_blending_backward(G["uv"], G["conic"], sc.opacity, feat, G["idx"], G["tr"], BG, W, H, fT, nc, g)


@pytest.mark.parametrize("abs_tap", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_single_frame(gpu, oracle_mod, C, abs_tap):
    import dptr.gs as gs
    import splatter_a_video_amd._lib as L
    o = oracle_mod
    R = _reference(o)
    sc, G, N = R["sc"], R["G"][0], R["sc"].N
    feat, res = R["fwd"][C]
    g = np.random.default_rng(40 + C).normal(size=(C, H, W)).astype(np.float32)
    idx, tr = gs.sort_gaussian(dev(G["uv"], gpu), dev(G["depth"], gpu), W, H, dev(G["radius"], gpu), dev(G["tiles"], gpu))
    assert (idx.cpu().numpy() == G["idx"]).all() and (tr.cpu().numpy() == G["tr"]).all()

    def run():
        t = {k: dev(v, gpu).requires_grad_(True) for k, v in dict(uv=G["uv"], conic=G["conic"], opacity=sc.opacity, feat=feat).items()}
        ndc = torch.zeros(N, 2, device=gpu, requires_grad=True)
        andc = torch.zeros(N, 2, device=gpu, requires_grad=True) if abs_tap else None
        out = gs.alpha_blending(t["uv"], t["conic"], t["opacity"], t["feat"], idx, tr, BG, W, H, ndc, andc)
        (out * dev(g, gpu)).sum().backward()
        torch.cuda.synchronize()
        return [out.detach(), t["uv"].grad, t["conic"].grad, t["opacity"].grad, t["feat"].grad, ndc.grad] + ([andc.grad] if abs_tap else [])

    assert not L.deterministic()
    L.set_deterministic(True)
    try:
        a, b = run(), run()
    finally:
        L.set_deterministic(False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    np.testing.assert_allclose(a[0].cpu().numpy(), res[0][0], rtol=IMG_RTOL, atol=IMG_ATOL)
    gr = _oracle_backward(o, R, C, 0, g)
    half = np.array([[0.5 * W, 0.5 * H]], np.float32)
    assert_grad(a[1], gr[0], "dL_duv")
    assert_grad(a[2], gr[1], "dL_dconic")
    assert_grad(a[3], gr[2], "dL_dopacity")
    assert_grad(a[4], gr[3], "dL_dfeature")
    assert_grad(a[5], gr[0] * half, "dL_dndc")
    if abs_tap:
        assert_grad(a[6], gr[4] * half, "dL_dabs_ndc")


@pytest.mark.parametrize("abs_tap", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_frame_batch(gpu, oracle_mod, C, abs_tap):
    import dptr.gs as gs
    from splatter_a_video_amd.frames import FrameBatch
    o = oracle_mod
    R = _reference(o)
    sc, N = R["sc"], R["sc"].N
    feat, res = R["fwd"][C]
    gv = np.random.default_rng(50 + C).normal(size=(F, C, H, W)).astype(np.float32)
    g = dev(gv, gpu)
    offv = np.zeros((F, N, 3), np.float32)
    offv[1, :, 0] = R["dxw"]
    off, extr = dev(offv, gpu), dev(sc.extr, gpu)

    def params():
        return {k: dev(v, gpu).requires_grad_(True) for k, v in dict(xyz=sc.xyz, scales=sc.scale, uquats=sc.rotate, opacity=sc.opacity,
                                                                     feat=feat).items()}

    def run():
        p = params()
        B = FrameBatch(F, N, W, H, C, "cuda", want_abs=abs_tap)
        out = B.render(p["xyz"], p["scales"], p["uquats"], p["opacity"], p["feat"], off, extr, bg=BG)
        torch.cuda.synchronize()
        words = B.cull_flags.cpu().numpy().copy()
        idx_b, tr_b = B.idx_sorted.cpu().numpy(), B.tile_range.cpu().numpy().reshape(F, -1, 2)
        out.backward(g)
        torch.cuda.synchronize()
        assert B.check() > 0
        return B, p, words, idx_b, tr_b, ([out.detach()] + [p[k].grad for k in p] + [B.tap.clone()] + ([B.abs_tap.clone()] if abs_tap else []))

    B, pb, words, idx_b, tr_b, a = run()
    b = run()[5]
    for x, y in zip(a, b):
        assert torch.equal(x, y)

    # the lists the kernel walked, counted from the batch's OWN tile lists and ncontrib (its binning may drop entries of the
    # oracle's lists that reach no pixel of a tile): they show the shapes above as well, and bit 8 w + q of an entry's cull word
    # says whether it applied in quarter q of wave w
    nc_b = B.ncontrib.cpu().numpy()
    for f in range(F):
        G = R["G"][f]
        mine = _lists(dict(G, idx=idx_b[f], tr=tr_b[f]), sc.opacity, nc_b[f])
        if f == 0:
            _assert_shapes(mine)
        for t, (n, app, _) in mine.items():
            if f == 0:      # the generator's count: the scene's own frame, where every entry of a planned tile applies in it
                n_o, app_o, _ = R["lists"][f][t]
                assert n == n_o and (app == app_o).all(), f"tile {t}: the batch's lists are not the oracle's"
            wt = words[f][int(tr_b[f][t, 0]):int(tr_b[f][t, 0]) + n].astype(np.uint32)
            bits = ((wt[:, None, None] >> (8 * np.arange(4)[None, :, None] + np.arange(4)[None, None, :]).astype(np.uint32)) & 1).astype(bool)
            assert (bits == app).all(), f"frame {f} tile {t}: the forward's applied bits differ from the counted lists"

    out = a[0].cpu().numpy()
    half = np.array([[0.5 * W, 0.5 * H]], np.float32)
    tap = atap = dop = dfe = 0.0
    for f in range(F):
        np.testing.assert_allclose(out[f], res[f][0], rtol=IMG_RTOL, atol=IMG_ATOL)
        gr = _oracle_backward(o, R, C, f, gv[f])
        tap, atap, dop, dfe = tap + gr[0] * half, atap + gr[4] * half, dop + gr[2], dfe + gr[3]
    assert_grad(B.tap, tap, "tap")
    if abs_tap:
        assert_grad(B.abs_tap, atap, "abs_tap")
    assert_grad(pb["opacity"].grad, dop, "dL_dopacity")
    assert_grad(pb["feat"].grad, dfe, "dL_dfeature")

    # d conic reaches the parameters through the projection chain: against the per-frame operators (same arithmetic per pair
    # record, other summation order over the frames: the bars of tests/test_gpu_frames.py)
    pa = params()
    for f in range(F):
        uv, depth, conic, radius, tiles = gs.preprocess_ortho(pa["xyz"], pa["scales"], pa["uquats"], extr, W, H, nearest=0.01, offset=off[f])
        idx, tr = gs.sort_gaussian(uv, depth, W, H, radius, tiles)
        img = gs.alpha_blending(uv, conic, pa["opacity"], pa["feat"], idx, tr, BG, W, H)
        assert torch.equal(img, a[0][f])
        (img * g[f]).sum().backward()
    for k in pa:
        x, y = pb[k].grad, pa[k].grad
        d = (x - y).abs()
        bad = d > 2e-4 * y.abs() + 2e-6 * float(y.abs().max()) + 1e-12
        assert int(bad.sum()) <= max(2, x.numel() // 100000), (k, int(bad.sum()))
        assert bool((d <= 2e-3 * y.abs() + 2e-5 * float(y.abs().max()) + 1e-12).all()), k
