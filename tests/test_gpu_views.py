"""Novel views and stereo on the GPU (splatter_a_video_amd.views; frame_preprocess_fwd_batch_cam_kernel, frames_present_kernel):
the dynamic frame batch under a camera per frame and under the pinhole camera against the CPU oracle frame by frame, one
orthographic camera as the bits of the single-camera kernel, the forward-only contract, the clip mechanics (batches,
capacity regrowth, fractional times, a wide set), and the display-ready bytes against tests/views_ref.py.

The scene is the one of tests/test_gpu_layers.py: 2001 dynamic Gaussians (not a multiple of the 64-quad block), 30 frames,
96 x 64.  At that size every frame is a grid.y slice of its own, so the four-frame trip of the kernel (lane k keeps frame
f + k and its camera) is exercised by one more test on 40000 Gaussians that needs no oracle: the batch against the same
kernel frame by frame (bits) and against the single-camera kernel (the project's uv / conic / radius rules)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle_chain as oc
import views_ref as VR
from test_gpu_frames_oracle import _rot_z
from test_gpu_layers import H, N, NAMES, TIMES, W, Scene, _dynamic_host, _t
from test_gpu_parity import IMG_ATOL, IMG_RTOL

pytestmark = pytest.mark.gpu

K = 4
NEAREST_PINHOLE = 0.2
FOCAL = (84.0, 80.0)              # pinhole focal lengths: see _intr


@pytest.fixture(scope="module")
def scene(gpu):
    sc = Scene()
    rng = np.random.default_rng(23)
    sc.attr_np = rng.uniform(-1, 1, size=(N, 2)).astype(np.float32)
    sc.attr = _t(sc.attr_np)
    sc.geo = {k: sc.model[k] for k in NAMES}
    return sc


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    R = np.eye(4, dtype=np.float32)
    R[1, 1], R[1, 2], R[2, 1], R[2, 2] = c, -s, s, c
    return R


def _cameras(F):
    """F world-to-camera matrices that all differ: a rotation about z, a tilt about x of a few degrees, a shift"""
    out = []
    for f in range(F):
        e = (_rot_x(np.deg2rad(3.0) * np.sin(1.0 + 2.0 * f)) @ _rot_z(0.09 * np.cos(0.5 + 1.3 * f))).astype(np.float32)
        e[0, 3], e[1, 3], e[2, 3] = 0.05 * np.sin(0.7 * f), -0.04 * np.cos(1.1 * f), 0.2 + 0.1 * np.sin(0.4 * f)
        out.append(e)
    return np.stack(out)


def _intr(F=None):
    """the pinhole camera: the Gaussians sit at |x|, |y| < 1.1 and 2 < z < 4, so a focal length of 84 pixels (the image half
    width over the tangent of a 30 degree half angle) keeps about 1900 of the 2001 in the 96 x 64 image, each with at least
    the pair of its own tile -- more than 1000 pairs a frame, which the test asserts; per frame it changes by a few percent"""
    k = np.array([FOCAL[0], FOCAL[1], W / 2 + 0.75, H / 2 - 0.5], np.float32)
    if F is None:
        return k
    return np.stack([k * np.array([1 + 0.03 * np.sin(f), 1 - 0.02 * np.cos(f), 1.0, 1.0], np.float32) for f in range(F)]).astype(np.float32)


def _np_sets(sc):
    return [dict(feature=sc.rgb_np, bg=1.0, taps=True), dict(feature="depth", bg=1.0),
            dict(feature=sc.attr_np, bg=0.0, detach_opacity=True)]


def _sets(sc):
    return [dict(feature=sc.rgb, bg=1.0, taps=True), dict(feature="depth", bg=1.0), dict(feature=sc.attr, bg=0.0, detach_opacity=True)]


def _oracle_frames(o, sc, times, extr, intr, nearest):
    """the oracle, frame by frame: dynamic_eval_forward, then the static chain under that frame's camera (zero image gradients)"""
    host = sc.host
    zero = [np.zeros((c, H, W), np.float32) for c in (3, 1, 2)]
    per = []
    for f, t in enumerate(times):
        seg, d, basis = sc.clock.scalars(t)
        b = np.array(list(basis), np.float32)
        pos, rot, opa, scl = o.dynamic_eval_forward(host["position"], host["pos_cubic_node"], host["rotation"], host["rot_poly_feat"],
                                                    host["rot_fourier_feat"], host["opacity"], host["scaling"], seg, d, b[:4], b[4:])
        e = extr[f] if np.ndim(extr) == 3 else extr
        k = None if intr is None else (intr[f] if np.ndim(intr) == 2 else intr)
        per.append(oc.frame(o, pos, scl, rot, opa, e, W, H, _np_sets(sc), zero, K, nearest=nearest, intr=k))
    return per


def _render(sc, times, extr, intr=None, nearest=0.01, **kw):
    from splatter_a_video_amd.frames import FrameBatch
    fb = FrameBatch(len(times), N, W, H, 6, "cuda")
    with torch.no_grad():
        res = fb.render_dynamic_sets(sc.clock, times, _t(extr), _sets(sc), K=K, nearest=nearest, intr=None if intr is None else _t(intr),
                                     **sc.geo, cubic_layout=0, **kw)
    torch.cuda.synchronize()
    fb.check()
    return fb, res


def _check_against_oracle(fb, res, per, name, min_pairs):
    """the project's rules (tests/test_gpu_frames_oracle.py): radius differs on <= 1e-4 of the Gaussians of a frame, uv within
    rtol 1e-5 / atol 2e-4, the conic within rtol 2e-5 / atol 2e-6 max|conic|, images within IMG_ATOL + IMG_RTOL |ref| on all
    but 1e-3 of a set's values per frame, ids differing on < 1e-3 of the pixels"""
    rad, uv, conic = fb.radius.cpu().numpy(), fb.uv.cpu().numpy(), fb.conic.cpu().numpy()
    pairs = fb.pairs.cpu().tolist()
    got = torch.cat(res[:3], 1).cpu().numpy()
    ids = res[-1].cpu().numpy()
    assert all(not t.requires_grad for t in res[:3])
    for f, r in enumerate(per):
        share = float((rad[f] != r["radius"]).mean())
        print(f"{name} frame {f}: {pairs[f]} pairs (oracle, full squares: {r['M']}), radius differs on {share:.2e}")
        assert pairs[f] > min_pairs, (name, f, pairs[f])
        assert share <= 1e-4, (name, f, share)
        np.testing.assert_allclose(uv[f], r["uv"], rtol=1e-5, atol=2e-4)
        same = rad[f] == r["radius"]
        np.testing.assert_allclose(conic[f][same], r["conic"][same], rtol=2e-5, atol=2e-6 * float(np.abs(r["conic"]).max()))
        c = 0
        for img, sname in zip(r["imgs"], ("rgb", "depth", "attribute")):
            a = got[f, c:c + img.shape[0]]
            bad = float((np.abs(a - img) > (IMG_ATOL + IMG_RTOL * np.abs(img))).mean())
            print(f"{name} frame {f} {sname}: {bad:.2e} of the values outside the image rule")
            assert bad < 1e-3, (name, f, sname, bad)
            c += img.shape[0]
        assert (ids[f] != r["gs_idx"]).any(-1).mean() < 1e-3, (name, f)
    assert float(np.abs(got[:, :3] - 1.0).max()) > 0.1            # something was composited


# ------------------------------------------------------------------ 1. a camera per frame, orthographic
@pytest.mark.parametrize("times", [TIMES, [7], [0, 1, 2, 5, 9, 14, 20, 26, 29]], ids=["F6", "F1", "F9"])
def test_per_frame_orthographic_cameras_against_the_oracle(oracle_mod, scene, times):
    extr = _cameras(len(times))
    fb, res = _render(scene, times, extr)
    per = _oracle_frames(oracle_mod, scene, times, extr, None, 0.01)
    _check_against_oracle(fb, res, per, f"ortho F={len(times)}", 100)


# ------------------------------------------------------------------ 2. the pinhole camera
@pytest.mark.parametrize("per_frame_intr", [False, True], ids=["intr4", "intrF4"])
def test_pinhole_cameras_against_the_oracle(oracle_mod, scene, per_frame_intr):
    extr = _cameras(len(TIMES))
    intr = _intr(len(TIMES) if per_frame_intr else None)
    fb, res = _render(scene, TIMES, extr, intr, nearest=NEAREST_PINHOLE)
    per = _oracle_frames(oracle_mod, scene, TIMES, extr, intr, NEAREST_PINHOLE)
    _check_against_oracle(fb, res, per, f"pinhole per_frame_intr={per_frame_intr}", 1000)


# ------------------------------------------------------------------ 3. one orthographic camera: the single-camera kernel
def _preprocess(sc, geo, n, tab, F, cam=None, extr=None, nearest=0.01):
    """one of the two batched dynamic preprocess entry points, straight through the binding"""
    import splatter_a_video_amd._lib as L
    lib = L.lib()
    I = sc.clock.interval_num
    o = dict(uv=torch.full((F, n, 2), -7.0, device="cuda"), depth=torch.full((F, n, 1), -7.0, device="cuda"),
             conic=torch.full((F, n, 3), -7.0, device="cuda"), radius=torch.full((F, n), -7, dtype=torch.int32, device="cuda"),
             opa_t=torch.full((n, 1), -7.0, device="cuda"))
    head = (F, n, I, L.ptr(tab), L.ptr(geo["position"]), L.ptr(geo["pos_cubic_node"]), 0, L.ptr(geo["rotation"]),
            L.ptr(geo["rot_poly_feat"]), L.ptr(geo["rot_fourier_feat"]), L.ptr(geo["opacity"]), L.ptr(geo["scaling"]))
    tail = (W, H, nearest, 1.3, L.ptr(o["uv"]), L.ptr(o["depth"]), L.ptr(o["conic"]), L.ptr(o["radius"]), L.ptr(o["opa_t"]), L.stream())
    if cam is None:
        L.check(lib.splat_frame_preprocess_forward_batch(*head, L.ptr(extr), *tail))
    else:
        L.check(lib.splat_frame_preprocess_forward_batch_cam(*head, ctypes.byref(cam.struct()), *tail))
    torch.cuda.synchronize()
    return o


def _assert_close_geometry(a, b, name):
    """two kernels may contract differently: the uv / conic / radius rules, no bit claim"""
    ra, rb = a["radius"].cpu().numpy(), b["radius"].cpu().numpy()
    for f in range(ra.shape[0]):
        assert (ra[f] != rb[f]).mean() <= 1e-4, (name, f)
    same = ra == rb
    np.testing.assert_allclose(a["uv"].cpu().numpy(), b["uv"].cpu().numpy(), rtol=1e-5, atol=2e-4)
    ca, cb = a["conic"].cpu().numpy(), b["conic"].cpu().numpy()
    np.testing.assert_allclose(ca[same], cb[same], rtol=2e-5, atol=2e-6 * float(np.abs(cb).max()))
    np.testing.assert_allclose(a["depth"].cpu().numpy(), b["depth"].cpu().numpy(), rtol=1e-5, atol=2e-4)


def test_one_orthographic_camera_is_the_single_camera_kernel(scene):
    from splatter_a_video_amd.dynamics import frame_table
    from splatter_a_video_amd.frames import FrameBatch, _Camera
    from splatter_a_video_amd.views import render_views
    F = len(TIMES)
    extr = _cameras(3)[2]
    e = _t(extr)
    tab = frame_table(scene.clock, TIMES, torch.device("cuda"))
    old = _preprocess(scene, scene.geo, N, tab, F, extr=e)
    new = _preprocess(scene, scene.geo, N, tab, F, cam=_Camera(e, None, F))
    for k in old:
        assert torch.equal(old[k], new[k]), k
    assert int((old["radius"] > 0).sum()) > 1000
    # F equal copies run the per-frame kernel: the same geometry within the rules
    copies = _preprocess(scene, scene.geo, N, tab, F, cam=_Camera(e[None].repeat(F, 1, 1).contiguous(), None, F))
    assert torch.equal(copies["opa_t"], old["opa_t"])
    _assert_close_geometry(copies, old, "equal copies")
    # through the public path: [4,4] is today's render_dynamic_sets (its buffers hold the old entry point's values), and
    # render_views with one camera is that path
    fb = FrameBatch(F, N, W, H, 6, "cuda")
    with torch.no_grad():
        res = fb.render_dynamic_sets(scene.clock, TIMES, e, _sets(scene), K=K, cubic_layout=0, **scene.geo)
    for k in ("uv", "depth", "conic", "radius"):
        assert torch.equal(getattr(fb, k), old[k]), k
    clip = render_views(scene.geo, scene.clock, TIMES, e, W, H, sets=_sets(scene), frames_per_batch=F, K=K)
    for got, want in zip((clip["set0"], clip["set1"], clip["set2"], clip["gs_idx"]), res):
        assert torch.equal(got, want)
    # a one-frame batch with a [1,4,4] camera takes the single-camera kernel too
    fb1 = FrameBatch(1, N, W, H, 6, "cuda")
    with torch.no_grad():
        one = fb1.render_dynamic_sets(scene.clock, TIMES[2:3], e[None].contiguous(), _sets(scene), K=K, cubic_layout=0, **scene.geo)
    for got, want in zip(one, res):
        assert torch.equal(got[0], want[2])


def test_four_frame_trips_and_unequal_slices():
    """40000 Gaussians: 625 blocks, so seven grid.y slices.  F = 9: slices of two frames and one of one; F = 30: trips of four
    frames and a last one of one.  Pinhole: the batch equals the same kernel run frame by frame (a one-frame batch keeps lane
    0 only), bit for bit.  Orthographic per-frame cameras: the single-camera kernel frame by frame, within the rules."""
    from splatter_a_video_amd.dynamics import frame_table
    from splatter_a_video_amd.frames import _Camera
    n, T = 40000, 30
    clock, host, _ = _dynamic_host(n, T, 9)

    class S:
        pass
    sc = S()
    sc.clock = clock
    geo = {k: _t(host[k]) for k in NAMES}
    dev = torch.device("cuda")
    for F in (9, 30):
        times = [float(t) for t in np.linspace(0, T - 1, F)]              # (fractional times)
        extr, intr = _t(_cameras(F)), _t(_intr(F))
        tab = frame_table(clock, times, dev)
        for persp in (True, False):
            cam = _Camera(extr, intr if persp else None, F)
            nearest = NEAREST_PINHOLE if persp else 0.01
            batch = _preprocess(sc, geo, n, tab, F, cam=cam, nearest=nearest)
            assert int((batch["radius"] > 0).sum(1).min()) > 10000
            assert float(batch["depth"].min()) >= 0.0 and int(batch["radius"].min()) >= 0      # every row was written
            for f in range(F):
                tab1 = frame_table(clock, times[f:f + 1], dev)
                if persp:
                    one = _preprocess(sc, geo, n, tab1, 1, cam=_Camera(extr[f:f + 1].contiguous(), intr[f:f + 1].contiguous(), 1),
                                      nearest=nearest)
                    for k in ("uv", "depth", "conic", "radius"):
                        assert torch.equal(batch[k][f], one[k][0]), (F, f, k)
                else:
                    one = _preprocess(sc, geo, n, tab1, 1, extr=extr[f].contiguous(), nearest=nearest)
                    _assert_close_geometry({k: batch[k][f:f + 1] for k in ("uv", "depth", "conic", "radius")}, one, (F, f))
                assert torch.equal(batch["opa_t"], one["opa_t"])


# ------------------------------------------------------------------ 4. forward only
def test_forward_only_contract(scene):
    from splatter_a_video_amd.frames import FrameBatch
    F = len(TIMES)
    fb = FrameBatch(F, N, W, H, 6, "cuda")
    extr = _t(_cameras(F))
    geo = dict(scene.geo)
    geo["position"] = scene.geo["position"].clone().requires_grad_(True)
    call = lambda e, **kw: fb.render_dynamic_sets(scene.clock, TIMES, e, _sets(scene), cubic_layout=0, **{**geo, **kw})
    with pytest.raises(ValueError, match="per-frame and pinhole cameras of a dynamic batch are forward only"):
        call(extr)
    with pytest.raises(ValueError, match="forward only"):
        call(extr[0].contiguous(), intr=_t(_intr()))
    rgb = scene.rgb.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="forward only"):
        fb.render_dynamic_sets(scene.clock, TIMES, extr, [dict(feature=rgb, bg=1.0, taps=True)] + _sets(scene)[1:], cubic_layout=0,
                               **scene.geo)
    with torch.no_grad():
        res = call(extr)
    assert all(not t.requires_grad for t in res[:3]) and res[-1] is None
    assert float((res[0] - 1.0).abs().max()) > 0.1
    # detached tensors render under grad mode
    res2 = fb.render_dynamic_sets(scene.clock, TIMES, extr, _sets(scene), cubic_layout=0, **scene.geo)
    assert all(torch.equal(a, b) for a, b in zip(res[:3], res2[:3]))
    # points= is not built for these cameras
    pts = dict(feature=scene.attr, points=torch.zeros(F, 2, device="cuda"), offsets=torch.arange(F + 1, device="cuda"), bg=0.0,
               detach_opacity=True)
    with pytest.raises(ValueError, match="points="):
        fb.render_dynamic_sets(scene.clock, TIMES, extr, _sets(scene), cubic_layout=0, points=pts, **scene.geo)
    # the one-camera path still backpropagates
    out = call(extr[0].contiguous())
    assert out[0].requires_grad
    (out[0].sum() + out[1].sum()).backward()
    g = geo["position"].grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0


# ------------------------------------------------------------------ 5. clip mechanics
def test_render_views_batches_capacity_and_fractional_times(scene):
    from splatter_a_video_amd.views import canonical_intrinsics, orbit_cameras, render_views
    T = 10
    times = [0, 3, 6.5, 9, 12, 14.25, 15, 22, 27.75, 29]
    orbit = orbit_cameras(T, radius=0.3, z_center=3.0, device="cuda")
    intr = _t(_intr())
    model = dict(scene.model)
    assert canonical_intrinsics(W, H).shape == (4,)
    # pinhole: one kernel serves every batch size, so batches of 4 (the last one partial) equal batches of 1 bit for bit
    st = {}
    a = render_views(model, scene.clock, times, orbit, W, H, intr=intr, frames_per_batch=4, nearest=NEAREST_PINHOLE, stats=st)
    b = render_views(model, scene.clock, times, orbit, W, H, intr=intr, frames_per_batch=1, nearest=NEAREST_PINHOLE)
    assert sorted(a) == ["depth", "mask_attribute", "rgb"] and st["regrows"] == 0
    for k, c in (("rgb", 3), ("depth", 1), ("mask_attribute", 1)):
        assert a[k].shape == (T, c, H, W) and not a[k].requires_grad
        assert torch.equal(a[k], b[k]), k
    assert float((a["rgb"] - 1.0).abs().amax(dim=(1, 2, 3)).min()) > 0.1          # every frame, the padded batch's too
    assert not torch.equal(a["rgb"][2], a["rgb"][3])
    # orthographic per-frame cameras: batches of 4 and of 3 run the same kernel
    c = render_views(model, scene.clock, times, orbit, W, H, frames_per_batch=4)
    d = render_views(model, scene.clock, times, orbit, W, H, frames_per_batch=3)
    assert all(torch.equal(c[k], d[k]) for k in c)
    # a deliberately tiny capacity: every batch is rendered again with a larger one, never returned short
    st = {}
    e = render_views(model, scene.clock, times, orbit, W, H, intr=intr, frames_per_batch=4, nearest=NEAREST_PINHOLE, capacity=64,
                     stats=st)
    assert st["regrows"] >= 1 and st["capacity"] > 1000
    assert all(torch.equal(a[k], e[k]) for k in a)
    # one camera for the whole clip at fractional times (the interpolated clip): frame 2 lies between its neighbours' times
    f = render_views(model, scene.clock, [6.0, 6.5, 7.0], orbit[0], W, H, frames_per_batch=2)
    assert f["rgb"].shape == (3, 3, H, W)
    assert not torch.equal(f["rgb"][1], f["rgb"][0]) and not torch.equal(f["rgb"][1], f["rgb"][2])


def test_render_views_wide_set_under_an_orbit(scene):
    from splatter_a_video_amd.frames import FrameBatch
    from splatter_a_video_amd.views import orbit_cameras, render_views
    F = len(TIMES)
    rng = np.random.default_rng(4)
    wide = dict(feature=_t(rng.uniform(-1, 1, size=(N, 40))), bg=0.0, detach_opacity=True)
    orbit = orbit_cameras(F, radius=0.3, z_center=3.0, device="cuda")
    out = render_views(scene.geo, scene.clock, TIMES, orbit, W, H, sets=_sets(scene), frames_per_batch=4, wide=wide)
    assert out["wide"].shape == (F, 40, H, W)
    fb = FrameBatch(F, N, W, H, 6, "cuda")
    with torch.no_grad():
        want = fb.render_dynamic_sets(scene.clock, TIMES, orbit, _sets(scene), cubic_layout=0, wide=wide, **scene.geo)
    for got, w_ in zip((out["set0"], out["set1"], out["set2"], out["wide"]), want):
        assert torch.equal(got, w_)
    assert float(out["wide"].abs().max()) > 0.1


# ------------------------------------------------------------------ 6. bytes
def test_to_uint8_is_clamp_times_255_truncated(gpu):
    from splatter_a_video_amd.views import to_uint8
    rng = np.random.default_rng(2)
    x = rng.uniform(-0.3, 1.3, size=(3, 3, 37, 29)).astype(np.float32)          # H * W = 1073: not a multiple of 4
    x[0, 0, 0, :] = np.arange(29, dtype=np.float32) * 8 / 255                   # exact k / 255
    x[1, :, 1, :4] = np.array([0.0, 1.0, -0.0, 254.5 / 255], np.float32)
    x[2, 1, 2, :3] = np.array([np.nan, np.inf, -np.inf], np.float32)
    x[2, 2, 36, 28] = np.nan                                                    # the very last pixel: the scalar tail
    t = torch.tensor(x, device="cuda")
    got = to_uint8(t)
    assert got.shape == (3, 37, 29, 3) and got.dtype == torch.uint8
    want = (torch.nan_to_num(t, nan=0.0).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1)
    assert torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), VR.to_uint8(x))
    # the aligned path (H * W a multiple of 4) and a non-contiguous input
    y = torch.tensor(rng.uniform(-0.3, 1.3, size=(2, 3, 6, 10)).astype(np.float32), device="cuda")
    assert torch.equal(to_uint8(y), (y.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1))
    z = y.flip(1)
    assert torch.equal(to_uint8(z), to_uint8(z.contiguous()))


def test_anaglyph_bytes_on_odd_and_aligned_shapes(gpu):
    from splatter_a_video_amd.views import ANAGLYPH, anaglyph
    rng = np.random.default_rng(8)
    custom = np.array([[0.9, 0.4, 0.0, 0.0, 0.0, 0.0], [0.0, -0.2, 0.0, 0.3, 0.8, 0.1], [0.0, 0.0, 0.0, 0.1, 0.2, 0.6]], np.float32)
    for shape in ((2, 3, 37, 29), (2, 3, 6, 10)):
        l = rng.uniform(-0.2, 1.2, size=shape).astype(np.float32)
        r = rng.uniform(-0.2, 1.2, size=shape).astype(np.float32)
        l[0, :, 0, :3] = np.array([np.nan, 1.0, 0.0], np.float32)
        for mode in list(ANAGLYPH) + [custom]:
            got = anaglyph(torch.tensor(l, device="cuda"), torch.tensor(r, device="cuda"), mode if isinstance(mode, str) else torch.tensor(mode))
            m = np.array(ANAGLYPH[mode], np.float32) if isinstance(mode, str) else mode
            assert np.array_equal(got.cpu().numpy(), VR.anaglyph(l, r, m)), (shape, mode if isinstance(mode, str) else "custom")


# ------------------------------------------------------------------ 7. the stereo clip
@pytest.mark.parametrize("pinhole", [False, True], ids=["ortho", "pinhole"])
def test_render_stereo(scene, pinhole):
    from splatter_a_video_amd.views import ANAGLYPH, render_stereo, render_views, stereo_cameras
    times = [0, 3.5, 14, 15, 29]
    eyes = stereo_cameras(radius=0.3, at_z=3.0, device="cuda")
    kw = dict(intr=_t(_intr()), nearest=NEAREST_PINHOLE) if pinhole else {}
    model = dict(scene.model)
    rgb_set = [dict(name="rgb", feature=scene.rgb, bg=1.0, taps=True)]
    # a row that sums above 1 saturates at 255
    custom = torch.tensor([[0.9, 0.8, 0.7, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
    got, left, right = render_stereo(model, scene.clock, times, W, H, cameras=eyes, mode="optimized", frames_per_batch=4,
                                     return_eyes=True, **kw)
    assert got.shape == (len(times), H, W, 3) and got.dtype == torch.uint8
    assert not torch.equal(left, right)
    for eye, img in zip(eyes, (left, right)):
        # "that camera alone": the pinhole camera has one kernel whatever the batch; an orthographic eye is given per frame, so
        # that it runs the per-frame kernel as the stereo batch does (the single-camera kernel may differ in the conic's last bit)
        cam = eye if pinhole else eye[None].repeat(len(times), 1, 1)
        alone = render_views(model, scene.clock, times, cam, W, H, sets=rgb_set, frames_per_batch=4, **kw)["rgb"]
        assert torch.equal(img, alone)
    l_np, r_np = left.cpu().numpy(), right.cpu().numpy()
    assert np.array_equal(got.cpu().numpy(), VR.anaglyph(l_np, r_np, np.array(ANAGLYPH["optimized"], np.float32)))
    for mode in ("true", custom):
        out = render_stereo(model, scene.clock, times, W, H, cameras=eyes, mode=mode, frames_per_batch=4, **kw)
        m = np.array(ANAGLYPH[mode], np.float32) if isinstance(mode, str) else mode.numpy()
        assert np.array_equal(out.cpu().numpy(), VR.anaglyph(l_np, r_np, m))
        if not isinstance(mode, str):
            assert int((out[..., 0] == 255).sum()) > 100 and float((l_np.clip(0, 1) * [[[0.9]], [[0.8]], [[0.7]]]).sum(1).max()) > 1.0
        else:
            assert int(out[..., 1].max()) == 0                                 # the "true" anaglyph has no green
