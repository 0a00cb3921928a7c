"""Layer editing on the GPU (splatter_a_video_amd.layers: frame_preprocess_fwd_layer_kernel, layer_centroid_*_kernel):
an untransformed layer is the compacted model bit for bit (the reference's render_part, src/trainer_fragGS.py:1310-1341),
copied / moved / resized layers against the CPU oracle on the numpy restatement of add_fg (:1344-1405, tests/layers_ref.py),
the per-frame centroids against a float64 mean, the clip mechanics (batches, capacity regrowth, cached tables) and the two
wrappers.  One scene for all tests: 2001 dynamic Gaussians, 30 frames, 96 x 64, six frame times (not a multiple of the
kernel's four-frame trip); the foreground x^2 + y^2 < 0.25 selects 345, so a copy makes Q = 2346 instances (not a multiple of
the 64-quad block)."""

import numpy as np
import pytest
import torch

import layers_ref as LR
import oracle_chain as oc
from test_gpu_parity import IMG_ATOL, IMG_RTOL

pytestmark = pytest.mark.gpu

N, T, W, H, SEED = 2001, 30, 96, 64, 5
TIMES = [0, 3, 14, 15, 22, 29]
DELAY = 2
LTIMES = [max(0, t - DELAY) for t in TIMES]
SCALE, DELTA = 0.6, (0.45, -0.3, -0.5)
DRIFT = (-0.004, 0.002, 0.003)
NAMES = ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")


def _t(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _dynamic_host(n, frames, seed):
    """the generator of the dynamic frame-batch oracle tests"""
    from splatter_a_video_amd.dynamics import FrameClock
    clock = FrameClock(frames)
    I = clock.interval_num
    rng = np.random.default_rng(seed)
    f = lambda *s, scale=1.0: rng.normal(0, scale, size=s).astype(np.float32)
    host = dict(position=np.concatenate([rng.uniform(-1.1, 1.1, size=(n, 2)), rng.uniform(2.0, 4.0, size=(n, 1))], 1).astype(np.float32),
                pos_cubic_node=f(n, 4 * I * 3, scale=0.02), rotation=f(n, 4), rot_poly_feat=f(n, 4, 4, scale=0.05),
                rot_fourier_feat=f(n, 8, 4, scale=0.05), opacity=f(n, 1, scale=1.5),
                scaling=np.log(rng.uniform(0.006, 0.03, size=(n, 3))).astype(np.float32))
    return clock, host, rng


class Scene:
    def __init__(self):
        from splatter_a_video_amd.renderer import OrthoEnhancedRenderer
        self.clock, self.host, rng = _dynamic_host(N, T, SEED)
        self.I = self.clock.interval_num
        p = self.host["position"]
        self.sel = (p[:, 0] ** 2 + p[:, 1] ** 2) < 0.25
        assert int(self.sel.sum()) == 345
        shs = rng.normal(0, 0.3, size=(N, 16, 3)).astype(np.float32)
        self.mask_np = np.where(self.sel, 0.9, 0.1).astype(np.float32)[:, None]
        self.model = {k: _t(v) for k, v in self.host.items()}
        self.model["shs"] = _t(shs)
        self.model["mask_attribute"] = _t(self.mask_np)
        self.rgb = OrthoEnhancedRenderer.colors(self.model["shs"]).detach()
        self.rgb_np = self.rgb.cpu().numpy()
        self.extr = torch.eye(4, device="cuda")
        self.sel_t = torch.tensor(self.sel, device="cuda")

    def sets(self, rgb=None, mask=None, bg=1.0):
        return [dict(feature=self.rgb if rgb is None else rgb, bg=bg, taps=True), dict(feature="depth", bg=1.0),
                dict(feature=self.model["mask_attribute"] if mask is None else mask, bg=0.0, detach_opacity=True)]

    def np_sets(self, feats, bg=1.0):
        return [dict(feature=feats[0], bg=bg, taps=True), dict(feature="depth", bg=1.0),
                dict(feature=feats[1], bg=0.0, detach_opacity=True)]

    def layout_model(self, layout):
        """the model dict with the spline table in ``layout``"""
        from splatter_a_video_amd.dynamics import SEGMENT_MAJOR, to_segment_major
        m = dict(self.model)
        if layout == SEGMENT_MAJOR:
            m["pos_cubic_node"] = to_segment_major(self.model["pos_cubic_node"], self.I)
        return m


@pytest.fixture(scope="module")
def scene(gpu):
    return Scene()


@pytest.fixture(scope="module")
def part_clips(scene):
    """test 1's single-layer clips (Gaussian-major table), rendered once: name -> (clip, images)"""
    from splatter_a_video_amd.layers import Layer, LayeredClip
    out = {}
    for name, sel in (("fg", scene.sel_t), ("bg", ~scene.sel_t)):
        clip = LayeredClip(scene.model, scene.clock, [Layer(select=sel)], scene.extr, W, H, scene.sets(), frames_per_batch=len(TIMES))
        out[name] = (clip, clip.render(TIMES))
    return out


def _copy_layers(scene, per_frame, which="copy", scale_splats=False):
    """the scenes of test 2 as (python layers, reference layers)"""
    from splatter_a_video_amd.layers import Layer
    lt = np.array(LTIMES, np.float32)[:, None]
    d_a = np.array(DELTA, np.float32)
    d_b = np.array((-0.5, 0.35, 0.4), np.float32)
    if per_frame:
        d_a = (d_a[None] + np.array(DRIFT, np.float32)[None] * lt).astype(np.float32)
        d_b = (d_b[None] - np.array(DRIFT, np.float32)[None] * lt).astype(np.float32)
    A = dict(select=scene.sel, times=LTIMES, scale=SCALE, delta=d_a, scale_splats=scale_splats)
    B = dict(select=scene.sel, times=LTIMES, scale=1.4, delta=d_b)
    ref = {"copy": [dict(select=None), A], "move": [dict(select=~scene.sel), A], "two copies": [dict(select=None), A, B]}[which]
    py = [Layer(select=None if l_["select"] is None else torch.tensor(l_["select"], device="cuda"), times=l_.get("times"),
                scale=l_.get("scale", 1.0), delta=l_.get("delta"), scale_splats=l_.get("scale_splats", False)) for l_ in ref]
    return py, ref


@pytest.fixture(scope="module")
def copy_clip(scene):
    """the "copy" scene with a [3] delta, rendered once (tests 2, 4 and 5 share it)"""
    from splatter_a_video_amd.layers import LayeredClip
    py, ref = _copy_layers(scene, False)
    clip = LayeredClip(scene.model, scene.clock, py, scene.extr, W, H, scene.sets(bg=0.0), frames_per_batch=len(TIMES))
    return clip, clip.render(TIMES), ref


# ------------------------------------------------------------------ 1. an untransformed layer is the compacted model
def _compact_reference(scene, sel, layout):
    """FrameBatch.render_dynamic_sets on the parameters indexed by the selection"""
    from splatter_a_video_amd.dynamics import SEGMENT_MAJOR, to_segment_major
    from splatter_a_video_amd.frames import FrameBatch
    m = {k: (scene.model[k] if sel is None else scene.model[k][sel]).contiguous() for k in NAMES}
    if layout == SEGMENT_MAJOR:
        m["pos_cubic_node"] = to_segment_major(m["pos_cubic_node"], scene.I)
    rgb = scene.rgb if sel is None else scene.rgb[sel].contiguous()
    mask = scene.model["mask_attribute"] if sel is None else scene.model["mask_attribute"][sel].contiguous()
    S = m["position"].shape[0]
    B = FrameBatch(len(TIMES), S, W, H, 5, "cuda")
    with torch.no_grad():
        res = B.render_dynamic_sets(scene.clock, TIMES, scene.extr, scene.sets(rgb, mask), cubic_layout=layout, **m)
    return B, res[:3]


def _assert_same_batch(fb, imgs, B, want):
    torch.cuda.synchronize()
    for name in ("uv", "depth", "conic", "radius", "tile_range", "pairs"):
        assert torch.equal(getattr(fb, name), getattr(B, name)), name
    pairs = B.pairs.cpu().tolist()
    assert min(pairs) > 100
    for f, m in enumerate(pairs):
        assert torch.equal(fb.idx_sorted[f, :m], B.idx_sorted[f, :m]), ("idx_sorted", f)
    for a, b, name in zip(imgs, want, ("rgb", "depth", "mask_attribute")):
        assert a.shape == b.shape and torch.equal(a, b), name


@pytest.mark.parametrize("layout", [0, 1], ids=["gaussian_major", "segment_major"])
@pytest.mark.parametrize("part", ["fg", "bg", "all"])
def test_untransformed_layer_is_the_compacted_model_bit_for_bit(scene, part_clips, part, layout):
    from splatter_a_video_amd.dynamics import GAUSSIAN_MAJOR, SEGMENT_MAJOR
    from splatter_a_video_amd.layers import Layer, LayeredClip
    assert (GAUSSIAN_MAJOR, SEGMENT_MAJOR) == (0, 1)
    sel = {"fg": scene.sel_t, "bg": ~scene.sel_t, "all": None}[part]
    if layout == GAUSSIAN_MAJOR and part in part_clips:
        clip, imgs = part_clips[part]
    else:
        clip = LayeredClip(scene.layout_model(layout), scene.clock, [Layer(select=sel)], scene.extr, W, H, scene.sets(),
                           frames_per_batch=len(TIMES), cubic_layout=layout)
        imgs = clip.render(TIMES)
    assert clip.Q == {"fg": 345, "bg": N - 345, "all": N}[part]
    B, want = _compact_reference(scene, sel, layout)
    _assert_same_batch(clip.fb, imgs, B, want)
    assert float((imgs[0] - 1.0).abs().max()) > 0.1       # something was composited


# ------------------------------------------------------------------ 2. copy and move against the oracle
def _check_against_oracle(o, scene, clip, imgs, ref_layers, name, bg=0.0):
    """the project's rules for a frame batch against the oracle chain: radius differs on <= 1e-4 of the instances per frame,
    uv within rtol 1e-5 / atol 2e-4, images within IMG_ATOL + IMG_RTOL |ref| on all but 1e-3 of a set's values per frame"""
    torch.cuda.synchronize()
    extr = np.eye(4, dtype=np.float32)
    rad, uv = clip.fb.radius.cpu().numpy(), clip.fb.uv.cpu().numpy()
    zero = [np.zeros((c, H, W), np.float32) for c in (3, 1, 1)]
    worst = dict(radius=0.0, image=0.0)
    for f in range(len(TIMES)):
        a = LR.frame_arrays(o, scene.clock, scene.host, ref_layers, TIMES, f, features=[scene.rgb_np, scene.mask_np])
        assert a["position"].shape[0] == clip.Q
        r = oc.frame(o, a["position"], a["scale"], a["rotation"], a["opacity"], extr, W, H, scene.np_sets(a["features"], bg), zero)
        share = float((rad[f] != r["radius"]).mean())
        worst["radius"] = max(worst["radius"], share)
        print(f"{name} frame {f}: radius differs on {share:.2e} of {clip.Q} instances, {r['M']} pairs")
        assert share <= 1e-4, (name, f, share)
        np.testing.assert_allclose(uv[f], r["uv"], rtol=1e-5, atol=2e-4)
        for img, want, sname in zip(imgs, r["imgs"], ("rgb", "depth", "mask_attribute")):
            got = img[f].cpu().numpy()
            bad = float((np.abs(got - want) > (IMG_ATOL + IMG_RTOL * np.abs(want))).mean())
            worst["image"] = max(worst["image"], bad)
            print(f"{name} frame {f} {sname}: {bad:.2e} of the values outside the image rule")
            assert bad < 1e-3, (name, f, sname, bad)
    return worst


def test_copy_against_the_oracle(oracle_mod, scene, copy_clip):
    clip, imgs, ref = copy_clip
    assert clip.Q == N + 345 == 2346
    _check_against_oracle(oracle_mod, scene, clip, imgs, ref, "copy [3]")
    # the copy is really composited: every copy visible in every frame, and the images differ from the unedited clip's
    rad = clip.fb.radius[:, N:]
    assert bool((rad > 0).all())
    from splatter_a_video_amd.layers import Layer, LayeredClip
    plain = LayeredClip(scene.model, scene.clock, [Layer()], scene.extr, W, H, scene.sets(bg=0.0), frames_per_batch=len(TIMES))
    base = plain.render(TIMES)
    assert float(((imgs[0] - base[0]).abs().amax(1) > 1e-3).float().mean()) > 0.03


@pytest.mark.parametrize("which,per_frame,scale_splats", [
    ("copy", True, False), ("copy", False, True), ("move", False, False), ("move", True, False), ("two copies", False, False),
    ("two copies", True, False)], ids=["copy-drift", "copy-scale_splats", "move", "move-drift", "two_copies", "two_copies-drift"])
def test_scenes_against_the_oracle(oracle_mod, scene, which, per_frame, scale_splats):
    from splatter_a_video_amd.layers import LayeredClip
    py, ref = _copy_layers(scene, per_frame, which, scale_splats)
    clip = LayeredClip(scene.model, scene.clock, py, scene.extr, W, H, scene.sets(bg=0.0), frames_per_batch=len(TIMES))
    imgs = clip.render(TIMES)
    assert clip.Q == {"copy": N + 345, "move": N, "two copies": N + 690}[which]
    _check_against_oracle(oracle_mod, scene, clip, imgs, ref, f"{which} drift={per_frame} scale_splats={scale_splats}")


# ------------------------------------------------------------------ 3. centroids
def _centroids(scene, tab, src, S, layout, cubic):
    import splatter_a_video_amd._lib as L
    lib = L.lib()
    F = tab.shape[0]
    nbytes = int(lib.splat_layer_centroids_scratch_bytes(F, S))
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    out = torch.full((F, 3), float("nan"), device="cuda")
    L.check(lib.splat_layer_centroids(F, N, S, scene.I, L.ptr(tab), L.ptr(src), L.ptr(scene.model["position"]), L.ptr(cubic), layout,
                                      L.ptr(out), L.ptr(scratch), nbytes, L.stream()))
    return out


@pytest.mark.parametrize("layout", [0, 1], ids=["gaussian_major", "segment_major"])
def test_layer_centroids(scene, layout):
    """within 2^-22 max|position| of the float64 mean of the positions operator's output: at most three roundings of difference
    between two evaluations of the spline expression plus the one rounding of the mean; the same bits on every run"""
    from splatter_a_video_amd.dynamics import frame_table, positions_batch_forward
    cubic = scene.layout_model(layout)["pos_cubic_node"]
    tab = frame_table(scene.clock, LTIMES, "cuda")
    pos = positions_batch_forward(tab, scene.model["position"], cubic, scene.I, layout)
    ids = torch.nonzero(scene.sel_t)[:, 0].to(torch.int32).contiguous()
    sel_pos = pos[:, scene.sel_t].double()
    bound = 2.0 ** -22 * float(sel_pos.abs().max())
    got = _centroids(scene, tab, ids, 345, layout, cubic)
    err = float((got.double() - sel_pos.mean(1)).abs().max())
    print(f"centroid of 345: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(got, _centroids(scene, tab, ids, 345, layout, cubic))
    one = ids[123:124].contiguous()
    got1 = _centroids(scene, tab, one, 1, layout, cubic)
    p1 = pos[:, int(one[0])].double()
    assert float((got1.double() - p1).abs().max()) <= 2.0 ** -22 * float(p1.abs().max())
    # every Gaussian in place (src == NULL) and a selection of more than one block of 1024
    every = _centroids(scene, tab, None, N, layout, cubic)
    assert float((every.double() - pos.double().mean(1)).abs().max()) <= 2.0 ** -22 * float(pos.abs().max())
    most = torch.nonzero(~scene.sel_t)[:, 0].to(torch.int32).contiguous()
    got_m = _centroids(scene, tab, most, N - 345, layout, cubic)
    assert float((got_m.double() - pos[:, ~scene.sel_t].double().mean(1)).abs().max()) <= 2.0 ** -22 * float(pos.abs().max())


# ------------------------------------------------------------------ 4. clip mechanics
def test_clip_batches_capacity_and_table_cache(scene):
    from splatter_a_video_amd.layers import LayeredClip
    import splatter_a_video_amd._lib as L
    times = TIMES + [7]                                   # seven frames, the last one out of order
    ltimes = [max(0, t - DELAY) for t in times]
    drift = (np.array(DELTA, np.float32)[None] + np.array(DRIFT, np.float32)[None] * np.array(ltimes, np.float32)[:, None])

    def layers():
        from splatter_a_video_amd.layers import Layer
        return [Layer(), Layer(select=scene.sel_t, times=ltimes, scale=SCALE, delta=drift)]
    make = lambda **k: LayeredClip(scene.model, scene.clock, layers(), scene.extr, W, H, scene.sets(bg=0.0), **k)
    whole = make(frames_per_batch=7)
    want = whole.render(times)
    assert whole.regrows == 0 and whole.table_builds == 2
    thirds = make(frames_per_batch=3)                     # 3 + 3 + 1: the last batch is padded with its frame and the padding dropped
    got = thirds.render(times)
    for a, b in zip(got, want):
        assert a.shape == (7, a.shape[1], H, W) and torch.equal(a, b)
    assert thirds.table_builds == 6
    # a later render of the same times reuses the cached tables
    keys = set(thirds._tables)
    again = thirds.render(times)
    assert thirds.table_builds == 6 and set(thirds._tables) == keys
    for a, b in zip(again, want):
        assert torch.equal(a, b)
    # a capacity far too small: the batch is rendered again with a larger one, never returned incomplete
    small = make(frames_per_batch=7, capacity=64)
    try:
        res = small.render(times)
    except L.SplatError as e:                             # (must not escape)
        pytest.fail(f"SplatError escaped: {e}")
    assert small.regrows >= 1 and small.fb.capacity >= int(small.fb.pairs.max())
    for a, b in zip(res, want):
        assert torch.equal(a, b)
    res2 = small.render(times)                            # and the object keeps working
    assert torch.equal(res2[0], want[0])


# ------------------------------------------------------------------ 5. wrappers
def test_render_part_is_the_single_layer_clip(scene, part_clips):
    from splatter_a_video_amd.layers import render_part
    for fg, name in ((True, "fg"), (False, "bg")):
        out = render_part(scene.model, scene.clock, TIMES, scene.extr, W, H, fg=fg, frames_per_batch=len(TIMES))
        assert list(out) == ["rgb", "depth", "mask_attribute"]
        for a, b in zip(out.values(), part_clips[name][1]):
            assert torch.equal(a, b), name
    # the mask and the colours as arguments; the default batches of eight frames
    m = {k: v for k, v in scene.model.items() if k not in ("shs", "mask_attribute")}
    out = render_part(m, scene.clock, TIMES, scene.extr, W, H, mask_attribute=scene.model["mask_attribute"][:, 0], shs=scene.model["shs"])
    assert torch.equal(out["rgb"], part_clips["fg"][1][0])


def test_add_foreground_is_the_copy_scene(scene, copy_clip):
    from splatter_a_video_amd.layers import add_foreground
    _, want, _ = copy_clip
    out = add_foreground(scene.model, scene.clock, TIMES, scene.extr, W, H, DELTA, SCALE, delay=DELAY, frames_per_batch=len(TIMES))
    for a, b in zip(out.values(), want):
        assert torch.equal(a, b)
    # a drift of zero is the same clip through the per-frame delta
    out = add_foreground(scene.model, scene.clock, TIMES, scene.extr, W, H, DELTA, SCALE, delay=DELAY, drift=(0.0, 0.0, 0.0))
    assert torch.equal(out["rgb"], want[0])
