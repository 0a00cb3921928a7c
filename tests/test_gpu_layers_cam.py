"""Layered clips under per-frame and pinhole cameras on the GPU (frame_preprocess_fwd_layer_cam_kernel behind
splat_frame_preprocess_layer_batch_cam, include/splat_hip_layers_cam.h; LayeredClip.render(extr=, intr=), render_part /
add_foreground, views.render_views / render_stereo with layers=, FrameBatch(records=False)).

The scene is the one of tests/test_gpu_layers.py (2001 dynamic Gaussians, 345 selected, 96 x 64, six frame times); the cameras
are those of tests/test_gpu_views.py (``_cameras``: all different; ``_intr``: the pinhole camera with nearest 0.2).  At that
size every frame is a grid.y slice of its own, so the four-frame trip of the kernel is exercised by one more test on 40000
instances that needs no oracle."""
import ctypes

import numpy as np
import pytest
import torch

import layers_ref as LR
import oracle_chain as oc
import views_ref as VR
from test_gpu_layers import DELAY, DELTA, DRIFT, H, LTIMES, N, NAMES, SCALE, TIMES, W, Scene, _copy_layers, _dynamic_host, _t
from test_gpu_parity import IMG_ATOL, IMG_RTOL
from test_gpu_views import NEAREST_PINHOLE, _assert_close_geometry, _cameras, _intr, _preprocess

pytestmark = pytest.mark.gpu

F6 = len(TIMES)
GEO = ("uv", "depth", "conic", "radius")


@pytest.fixture(scope="module")
def scene(gpu):
    sc = Scene()
    sc.geo = {k: sc.model[k] for k in NAMES}
    sc.ids = torch.nonzero(sc.sel_t)[:, 0].to(torch.int32).contiguous()
    return sc


def _centroids(geo, P, I, tab, src, S):
    import splatter_a_video_amd._lib as L
    lib = L.lib()
    F = tab.shape[0]
    nbytes = int(lib.splat_layer_centroids_scratch_bytes(F, S))
    scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device="cuda")
    out = torch.full((F, 3), float("nan"), device="cuda")
    L.check(lib.splat_layer_centroids(F, P, S, I, L.ptr(tab), L.ptr(src), L.ptr(geo["position"]), L.ptr(geo["pos_cubic_node"]), 0,
                                      L.ptr(out), L.ptr(scratch), nbytes, L.stream()))
    return out


def _layer_pre(geo, P, I, tab, F, S, Q, q0, src, cam=None, extr=None, centroid=None, delta=None, scale=1.0, splats=0, nearest=0.01):
    """one of the two layer preprocess entry points, straight through the binding, into buffers pre-filled with -7"""
    import splatter_a_video_amd._lib as L
    lib = L.lib()
    o = dict(uv=torch.full((F, Q, 2), -7.0, device="cuda"), depth=torch.full((F, Q, 1), -7.0, device="cuda"),
             conic=torch.full((F, Q, 3), -7.0, device="cuda"), radius=torch.full((F, Q), -7, dtype=torch.int32, device="cuda"),
             opa_t=torch.full((Q, 1), -7.0, device="cuda"))
    head = (F, P, S, Q, q0, I, L.ptr(tab), L.ptr(src), L.ptr(geo["position"]), L.ptr(geo["pos_cubic_node"]), 0, L.ptr(geo["rotation"]),
            L.ptr(geo["rot_poly_feat"]), L.ptr(geo["rot_fourier_feat"]), L.ptr(geo["opacity"]), L.ptr(geo["scaling"]))
    tail = (W, H, nearest, 1.3, L.ptr(centroid), L.ptr(delta), scale, splats, L.ptr(o["uv"]), L.ptr(o["depth"]), L.ptr(o["conic"]),
            L.ptr(o["radius"]), L.ptr(o["opa_t"]), L.stream())
    if cam is None:
        L.check(lib.splat_frame_preprocess_layer_batch(*head, L.ptr(extr), *tail))
    else:
        L.check(lib.splat_frame_preprocess_layer_batch_cam(*head, ctypes.byref(cam.struct()), *tail))
    torch.cuda.synchronize()
    return o


def _drift(F):
    lt = np.arange(F, dtype=np.float32)[:, None]
    return _t((np.array(DELTA, np.float32)[None] + np.array(DRIFT, np.float32)[None] * lt).astype(np.float32))


# ------------------------------------------------------------------ 1. dispatch: one orthographic camera is the old entry point
def test_one_orthographic_camera_dispatches_to_the_layer_entry_point(scene):
    from splatter_a_video_amd.dynamics import frame_table
    from splatter_a_video_amd.frames import _Camera
    I = scene.I
    e = _t(_cameras(3)[2])
    tab = frame_table(scene.clock, TIMES, torch.device("cuda"))
    cen = _centroids(scene.geo, N, I, tab, scene.ids, 345)
    delta = _drift(F6)
    cases = [dict(), dict(centroid=cen, delta=delta, scale=0.6, splats=0), dict(centroid=cen, delta=delta, scale=0.6, splats=1)]
    for kw in cases:
        old = _layer_pre(scene.geo, N, I, tab, F6, 345, 345, 0, scene.ids, extr=e, **kw)
        new = _layer_pre(scene.geo, N, I, tab, F6, 345, 345, 0, scene.ids, cam=_Camera(e, None, F6), **kw)
        for k in old:
            assert torch.equal(old[k], new[k]), (k, sorted(kw))
        assert int((old["radius"] > 0).sum(1).min()) > 100 and float(old["depth"].min()) >= 0.0
    plain, moved, sized = [_layer_pre(scene.geo, N, I, tab, F6, 345, 345, 0, scene.ids, extr=e, **kw) for kw in cases]
    assert not torch.equal(plain["uv"], moved["uv"]) and torch.equal(moved["uv"], sized["uv"])
    assert not torch.equal(moved["conic"], sized["conic"])                    # scale_splats reaches the covariance
    # a [1,4,4] camera with F = 1 is one camera too
    tab1 = frame_table(scene.clock, TIMES[2:3], torch.device("cuda"))
    for kw in (dict(), dict(centroid=cen[2:3].contiguous(), delta=delta[2:3].contiguous(), scale=0.6, splats=1)):
        old = _layer_pre(scene.geo, N, I, tab1, 1, 345, 345, 0, scene.ids, extr=e, **kw)
        new = _layer_pre(scene.geo, N, I, tab1, 1, 345, 345, 0, scene.ids, cam=_Camera(e[None].contiguous(), None, 1), **kw)
        for k in old:
            assert torch.equal(old[k], new[k]), (k, "F = 1")


# ------------------------------------------------------------------ 2. an untransformed layer is the plain cam kernel
@pytest.mark.parametrize("pinhole", [False, True], ids=["ortho", "pinhole"])
def test_untransformed_layer_against_the_plain_cam_kernel(scene, pinhole):
    """two kernels that may contract differently: opa_t bit for bit, the geometry by the project's rules, no bit claim"""
    from splatter_a_video_amd.dynamics import frame_table
    from splatter_a_video_amd.frames import _Camera
    tab = frame_table(scene.clock, TIMES, torch.device("cuda"))
    cam = _Camera(_t(_cameras(F6)), _t(_intr(F6)) if pinhole else None, F6)
    nearest = NEAREST_PINHOLE if pinhole else 0.01
    every = _layer_pre(scene.geo, N, scene.I, tab, F6, N, N, 0, None, cam=cam, nearest=nearest)
    want = _preprocess(scene, scene.geo, N, tab, F6, cam=cam, nearest=nearest)
    assert int((want["radius"] > 0).sum(1).min()) > 1000 and int((every["radius"] > 0).sum(1).min()) > 1000
    assert torch.equal(every["opa_t"], want["opa_t"])
    _assert_close_geometry(every, want, "all Gaussians")
    # a selected layer is that entry point on the compacted parameters
    part = _layer_pre(scene.geo, N, scene.I, tab, F6, 345, 345, 0, scene.ids, cam=cam, nearest=nearest)
    compact = {k: scene.model[k][scene.sel_t].contiguous() for k in NAMES}
    want = _preprocess(scene, compact, 345, tab, F6, cam=cam, nearest=nearest)
    assert int((want["radius"] > 0).sum(1).min()) > 100
    assert torch.equal(part["opa_t"], want["opa_t"])
    _assert_close_geometry(part, want, "selected")


# ------------------------------------------------------------------ 3. trips and slices
@pytest.mark.parametrize("pinhole", [True, False], ids=["pinhole", "ortho"])
def test_four_frame_trips_and_unequal_slices(gpu, pinhole):
    """40000 instances (every second of 80000 Gaussians): 625 blocks, so seven grid.y slices.  F = 9: slices of two frames and one
    of one; F = 30: trips of four frames and a last one of one.  Transformed, with a per-frame delta.  Pinhole: the batch equals
    the same entry point run one frame at a time, bit for bit.  Orthographic per-frame cameras: a one-frame call dispatches to
    the single-camera kernel, so the project's geometry rules.  Rows outside q0 .. q0 + S keep their -7."""
    from splatter_a_video_amd.dynamics import frame_table
    from splatter_a_video_amd.frames import _Camera
    P, T, S, q0 = 80000, 30, 40000, 100
    Q = q0 + S + 50
    clock, host, _ = _dynamic_host(P, T, 9)
    I = clock.interval_num
    geo = {k: _t(host[k]) for k in NAMES}
    src = torch.arange(0, P, 2, dtype=torch.int32, device="cuda")
    dev = torch.device("cuda")
    nearest = NEAREST_PINHOLE if pinhole else 0.01
    for F in (9, 30):
        times = [float(t) for t in np.linspace(0, T - 1, F)]              # (fractional times)
        extr, intr = _t(_cameras(F)), _t(_intr(F))
        tab = frame_table(clock, times, dev)
        cen, delta = _centroids(geo, P, I, tab, src, S), _drift(F)
        kw = dict(scale=0.6, splats=1, nearest=nearest)
        batch = _layer_pre(geo, P, I, tab, F, S, Q, q0, src, cam=_Camera(extr, intr if pinhole else None, F), centroid=cen,
                           delta=delta, **kw)
        rows = slice(q0, q0 + S)
        assert int((batch["radius"][:, rows] > 0).sum(1).min()) > 10000
        assert float(batch["depth"][:, rows].min()) >= 0.0 and int(batch["radius"][:, rows].min()) >= 0      # every row was written
        assert bool((batch["conic"][:, rows] != -7.0).all())
        assert float(batch["opa_t"][rows].min()) > 0.0
        for k in GEO:
            assert bool((batch[k][:, :q0] == -7).all()) and bool((batch[k][:, q0 + S:] == -7).all()), (F, k)
        assert bool((batch["opa_t"][:q0] == -7).all()) and bool((batch["opa_t"][q0 + S:] == -7).all())
        for f in range(F):
            tab1 = frame_table(clock, times[f:f + 1], dev)
            cam1 = _Camera(extr[f:f + 1].contiguous(), intr[f:f + 1].contiguous() if pinhole else None, 1)
            one = _layer_pre(geo, P, I, tab1, 1, S, Q, q0, src, cam=cam1, centroid=cen[f:f + 1].contiguous(),
                             delta=delta[f:f + 1].contiguous(), **kw)
            if pinhole:
                for k in GEO:
                    assert torch.equal(batch[k][f], one[k][0]), (F, f, k)
            else:
                _assert_close_geometry({k: batch[k][f:f + 1, rows] for k in GEO}, {k: one[k][:, rows] for k in GEO}, (F, f))
            assert torch.equal(batch["opa_t"], one["opa_t"])


# ------------------------------------------------------------------ 4. layered scenes under cameras against the oracle
def _check_against_oracle(o, scene, clip, imgs, ref_layers, name, extr, intr, nearest, bg=0.0):
    """the rules of tests/test_gpu_layers.py::_check_against_oracle under frame f's camera: radius differs on <= 1e-4 of the
    instances per frame, uv within rtol 1e-5 / atol 2e-4, images within IMG_ATOL + IMG_RTOL |ref| on all but 1e-3 of a set's
    values per frame; more than 3000 pairs in every frame"""
    torch.cuda.synchronize()
    rad, uv = clip.fb.radius.cpu().numpy(), clip.fb.uv.cpu().numpy()
    zero = [np.zeros((c, H, W), np.float32) for c in (3, 1, 1)]
    for f in range(F6):
        a = LR.frame_arrays(o, scene.clock, scene.host, ref_layers, TIMES, f, features=[scene.rgb_np, scene.mask_np])
        assert a["position"].shape[0] == clip.Q
        r = oc.frame(o, a["position"], a["scale"], a["rotation"], a["opacity"], extr[f], W, H, scene.np_sets(a["features"], bg), zero,
                     nearest=nearest, intr=None if intr is None else intr[f])
        share = float((rad[f] != r["radius"]).mean())
        print(f"{name} frame {f}: radius differs on {share:.2e} of {clip.Q} instances, {r['M']} pairs")
        assert r["M"] > 3000, (name, f, r["M"])
        assert share <= 1e-4, (name, f, share)
        np.testing.assert_allclose(uv[f], r["uv"], rtol=1e-5, atol=2e-4)
        for img, want, sname in zip(imgs, r["imgs"], ("rgb", "depth", "mask_attribute")):
            got = img[f].cpu().numpy()
            bad = float((np.abs(got - want) > (IMG_ATOL + IMG_RTOL * np.abs(want))).mean())
            print(f"{name} frame {f} {sname}: {bad:.2e} of the values outside the image rule")
            assert bad < 1e-3, (name, f, sname, bad)


@pytest.mark.parametrize("pinhole", [False, True], ids=["ortho", "pinhole"])
@pytest.mark.parametrize("which,scale_splats", [("copy", False), ("move", False), ("two copies", False), ("copy", True)],
                         ids=["copy", "move", "two_copies", "copy-scale_splats"])
def test_scenes_under_cameras_against_the_oracle(oracle_mod, scene, which, scale_splats, pinhole):
    from splatter_a_video_amd.layers import LayeredClip
    py, ref = _copy_layers(scene, True, which, scale_splats)
    extr, intr = _cameras(F6), (_intr(F6) if pinhole else None)
    nearest = NEAREST_PINHOLE if pinhole else 0.01
    clip = LayeredClip(scene.model, scene.clock, py, scene.extr, W, H, scene.sets(bg=0.0), frames_per_batch=F6, nearest=nearest)
    imgs = clip.render(TIMES, extr=_t(extr), intr=None if intr is None else _t(intr))
    assert clip.Q == {"copy": N + 345, "move": N, "two copies": N + 690}[which]
    _check_against_oracle(oracle_mod, scene, clip, imgs, ref, f"{which} scale_splats={scale_splats} pinhole={pinhole}", extr, intr,
                          nearest)
    if which == "copy":
        assert bool((clip.fb.radius[:, N:] > 0).all())                       # every copy instance is visible in every frame
    # the cameras really are per frame: the same clip under the first camera alone differs
    first = clip.render(TIMES, extr=_t(extr[0]), intr=None if intr is None else _t(intr[0]))
    assert torch.equal(first[0][0], imgs[0][0]) or not pinhole               # (frame 0 has that camera; ortho: another kernel)
    assert float(((first[0][1:] - imgs[0][1:]).abs().amax(1) > 1e-3).float().mean()) > 0.03


# ------------------------------------------------------------------ 5. clip mechanics
@pytest.mark.parametrize("pinhole", [False, True], ids=["ortho", "pinhole"])
def test_clip_batches_padding_and_capacity_under_cameras(scene, pinhole):
    from splatter_a_video_amd.layers import Layer, LayeredClip
    import splatter_a_video_amd._lib as L
    times = TIMES + [7]                                   # seven frames, the last one out of order
    ltimes = [max(0, t - DELAY) for t in times]
    drift = (np.array(DELTA, np.float32)[None] + np.array(DRIFT, np.float32)[None] * np.array(ltimes, np.float32)[:, None])
    extr = _t(_cameras(7))
    kw = dict(intr=_t(_intr(7)), nearest=NEAREST_PINHOLE) if pinhole else {}
    cams = dict(extr=extr, intr=kw.get("intr"))
    layers = lambda: [Layer(), Layer(select=scene.sel_t, times=ltimes, scale=SCALE, delta=drift)]
    make = lambda **k: LayeredClip(scene.model, scene.clock, layers(), scene.extr, W, H, scene.sets(bg=0.0),
                                   nearest=kw.get("nearest", 0.01), **k)
    whole = make(frames_per_batch=7)
    want = whole.render(times, **cams)
    assert whole.regrows == 0 and whole.fb.pair_records is None
    assert float((want[0] - 0.0).abs().amax(dim=(1, 2, 3)).min()) > 0.1
    thirds = make(frames_per_batch=3)                     # 3 + 3 + 1: the last batch is padded with its frame and camera
    got = thirds.render(times, **cams)
    for a, b in zip(got, want):
        assert a.shape == (7, a.shape[1], H, W) and torch.equal(a, b)
    small = make(frames_per_batch=7, capacity=64)         # a capacity far too small: rendered again, never returned incomplete
    try:
        res = small.render(times, **cams)
    except L.SplatError as e:                             # (must not escape)
        pytest.fail(f"SplatError escaped: {e}")
    assert small.regrows >= 1 and small.fb.capacity >= int(small.fb.pairs.max())
    for a, b in zip(res, want):
        assert torch.equal(a, b)
    # one camera for all frames through the call, and the same camera as the clip's default, are the same clip
    if pinhole:
        one = make(frames_per_batch=7).render(times, extr=extr[3], intr=cams["intr"][3])
        dflt = LayeredClip(scene.model, scene.clock, layers(), extr[3], W, H, scene.sets(bg=0.0), nearest=NEAREST_PINHOLE,
                           frames_per_batch=7, intr=cams["intr"][3]).render(times)
        for a, b in zip(one, dflt):
            assert torch.equal(a, b)
        assert torch.equal(one[0][3], want[0][3]) and not torch.equal(one[0][4], want[0][4])


def test_default_call_and_wrappers(scene):
    from splatter_a_video_amd.layers import Layer, LayeredClip, add_foreground, render_part
    # without cameras, a clip built without intr is today's clip: render_part's bits
    clip = LayeredClip(scene.model, scene.clock, [Layer(select=scene.sel_t)], scene.extr, W, H, scene.sets(), frames_per_batch=F6)
    assert clip.camera is None
    plain = clip.render(TIMES)
    out = render_part(scene.model, scene.clock, TIMES, scene.extr, W, H, frames_per_batch=F6)
    for a, b in zip(out.values(), plain):
        assert torch.equal(a, b)
    again = clip.render(TIMES, extr=scene.extr)           # the one orthographic camera through the new entry point: its dispatch
    for a, b in zip(again, plain):
        assert torch.equal(a, b)
    # the wrappers under [T,4,4] + intr are the LayeredClip they stand for
    extr, intr = _t(_cameras(F6)), _t(_intr(F6))
    for i_ in (intr, intr[0].contiguous(), None):
        nearest = 0.01 if i_ is None else NEAREST_PINHOLE
        out = render_part(scene.model, scene.clock, TIMES, extr, W, H, frames_per_batch=4, intr=i_, nearest=nearest)
        want = LayeredClip(scene.model, scene.clock, [Layer(select=scene.sel_t)], scene.extr, W, H, scene.sets(), frames_per_batch=4,
                           nearest=nearest).render(TIMES, extr=extr, intr=i_)
        assert list(out) == ["rgb", "depth", "mask_attribute"]
        for a, b in zip(out.values(), want):
            assert torch.equal(a, b)
        assert float((out["rgb"] - 1.0).abs().amax(dim=(1, 2, 3)).min()) > 0.1
        out = add_foreground(scene.model, scene.clock, TIMES, extr, W, H, DELTA, SCALE, delay=DELAY, frames_per_batch=4, intr=i_,
                             nearest=nearest)
        layers = [Layer(), Layer(select=scene.sel_t, times=LTIMES, scale=SCALE, delta=DELTA)]
        want = LayeredClip(scene.model, scene.clock, layers, scene.extr, W, H, scene.sets(bg=0.0), frames_per_batch=4,
                           nearest=nearest).render(TIMES, extr=extr, intr=i_)
        for a, b in zip(out.values(), want):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ 6. views
def test_render_views_of_the_whole_model_as_a_layer(scene):
    """the same model through two kernels: the image rule"""
    from splatter_a_video_amd.layers import Layer
    from splatter_a_video_amd.views import render_views
    extr = _t(_cameras(F6))
    for kw in (dict(), dict(intr=_t(_intr(F6)), nearest=NEAREST_PINHOLE)):
        st = {}
        got = render_views(scene.model, scene.clock, TIMES, extr, W, H, layers=[Layer()], frames_per_batch=4, stats=st, **kw)
        want = render_views(scene.model, scene.clock, TIMES, extr, W, H, frames_per_batch=4, **kw)
        assert sorted(got) == sorted(want) == ["depth", "mask_attribute", "rgb"] and st["regrows"] == 0 and st["capacity"] > 1000
        for k in want:
            a, b = got[k].cpu().numpy(), want[k].cpu().numpy()
            assert a.shape == b.shape == (F6, 3 if k == "rgb" else 1, H, W)
            for f in range(F6):
                bad = float((np.abs(a[f] - b[f]) > (IMG_ATOL + IMG_RTOL * np.abs(b[f]))).mean())
                assert bad < 1e-3, (k, f, bad)
        assert float((got["rgb"] - 1.0).abs().amax(dim=(1, 2, 3)).min()) > 0.1


@pytest.mark.parametrize("pinhole", [False, True], ids=["ortho", "pinhole"])
def test_render_stereo_of_a_layered_scene(scene, pinhole):
    """an eye of the stereo clip is render_views(layers=...) under that eye repeated per frame -- the same kernel, and frames are
    independent -- bit for bit (only the colours are composited, as in tests/test_gpu_views.py::test_render_stereo); the bytes
    are tests/views_ref.py's anaglyph of the eyes"""
    from splatter_a_video_amd.views import ANAGLYPH, render_stereo, render_views, stereo_cameras
    py, _ = _copy_layers(scene, True)
    eyes = stereo_cameras(radius=0.3, at_z=3.0, device="cuda")
    kw = dict(intr=_t(_intr()), nearest=NEAREST_PINHOLE) if pinhole else {}
    model = dict(scene.model)
    rgb_set = [dict(name="rgb", feature=scene.rgb, bg=1.0, taps=True)]
    got, left, right = render_stereo(model, scene.clock, TIMES, W, H, cameras=eyes, mode="optimized", frames_per_batch=4,
                                     return_eyes=True, layers=py, **kw)
    assert got.shape == (F6, H, W, 3) and got.dtype == torch.uint8 and not torch.equal(left, right)
    plain = render_stereo(model, scene.clock, TIMES, W, H, cameras=eyes, frames_per_batch=4, return_eyes=True, **kw)
    assert float(((left - plain[1]).abs().amax(1) > 1e-3).float().mean()) > 0.01          # the copy is in the picture
    for eye, img in zip(eyes, (left, right)):
        alone = render_views(model, scene.clock, TIMES, eye[None].repeat(F6, 1, 1), W, H, sets=rgb_set, frames_per_batch=4, layers=py,
                             **kw)["rgb"]
        assert torch.equal(img, alone)
    want = VR.anaglyph(left.cpu().numpy(), right.cpu().numpy(), np.array(ANAGLYPH["optimized"], np.float32))
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------ 7. the forward-only batch
def test_forward_only_batch(scene):
    from splatter_a_video_amd.frames import FrameBatch
    from splatter_a_video_amd.views import render_views
    cap = 20000
    full = FrameBatch(F6, N, W, H, 5, "cuda", capacity=cap)
    lean = FrameBatch(F6, N, W, H, 5, "cuda", capacity=cap, records=False)
    assert full.records and not lean.records and lean.pair_records is None
    assert full.pair_records.numel() == F6 * cap * full.ncp
    assert full.memory_bytes() - lean.memory_bytes() == F6 * cap * full.ncp * 4
    with torch.no_grad():
        a = full.render_dynamic_sets(scene.clock, TIMES, scene.extr, scene.sets(), cubic_layout=0, **scene.geo)
        b = lean.render_dynamic_sets(scene.clock, TIMES, scene.extr, scene.sets(), cubic_layout=0, **scene.geo)
    full.check(), lean.check()
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    assert float((a[0] - 1.0).abs().max()) > 0.1
    geo = dict(scene.geo, position=scene.geo["position"].clone().requires_grad_(True))
    gen = lean.generation
    with pytest.raises(ValueError, match="records=False"):
        lean.render_dynamic_sets(scene.clock, TIMES, scene.extr, scene.sets(), cubic_layout=0, **geo)
    with pytest.raises(ValueError, match="records=False"):
        lean.render_dynamic_sets(scene.clock, TIMES, scene.extr, scene.sets(), cubic_layout=0, differentiable=True, **scene.geo)
    assert lean.generation == gen                                              # refused before any launch
    out = full.render_dynamic_sets(scene.clock, TIMES, scene.extr, scene.sets(), cubic_layout=0, **geo)
    out[0].sum().backward()                                                    # the default batch still backpropagates
    assert float(geo["position"].grad.abs().sum()) > 0
    # the clip renderers build theirs without the records: the stats show the drop
    st = {}
    render_views(scene.model, scene.clock, TIMES, scene.extr, W, H, frames_per_batch=F6, stats=st)
    c = st["capacity"]
    with_records = FrameBatch(F6, N, W, H, 5, "cuda", capacity=c).memory_bytes()
    without = FrameBatch(F6, N, W, H, 5, "cuda", capacity=c, records=False).memory_bytes()
    assert without <= st["frame_batch_bytes"] <= without + 4                   # (+ the pinned overflow word, once a batch ran)
    assert with_records - without == F6 * c * full.ncp * 4 and st["frame_batch_bytes"] < with_records
