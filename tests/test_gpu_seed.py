"""Seeding the dynamic Gaussians on the GPU (splatter_a_video_amd/seed.py over csrc/seed.hip) against the reference's own
results in tests/golden/seed_clip.npz (tests/golden/make_golden_seed.py: the reference's median_filter_2d,
get_tracks_3d_for_query_frame and extend_track3d, and scipy's CubicSpline) and against torch / scipy computed here.

Bounds (eps = 2^-23):
* median: a selection, bit-equal;
* lifting: decisions identical (the generator keeps every decision clear of its threshold); x, y within 4 eps; depth and
  colours within 8 eps * max |value| (four products and three sums rounded once each, plus the two weight factors);
  confidences within 4e-7 (device exp within 2 ulp through a sigmoid bounded by 1);
* spline: |c_k - ref_k| <= eps |ref_k| + 1e-10 max|y| / h^(3-k) per segment of width h against scipy in float64 on the same
  float32 inputs -- one float32 rounding plus a cap that separates a float64 solve from a float32 one (a float32 Thomas solve
  misses it by four orders of magnitude)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import seed
from splatter_a_video_amd.dynamics import DynamicGaussians, FrameClock

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
HERE = os.path.dirname(os.path.abspath(__file__))
MED_TILE = (8, 32)      # rows x columns of the median kernel's output tile (csrc/seed.hip: MED_TY, MED_TX)


@pytest.fixture(scope="module")
def clip():
    return dict(np.load(os.path.join(HERE, "golden", "seed_clip.npz")))


def _t(a, dtype=np.float32):
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _raw_depth(clip):
    return (1.0 / np.clip(clip["disp"], 1e-6, 1e6)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ median
def test_median_11_is_the_references_bit_for_bit(gpu, clip):
    got = seed.median_filter_2d(_t(_raw_depth(clip)), 11)
    ref = torch.from_numpy(clip["depth_med"])
    assert got.shape == ref.shape and torch.equal(_bits(got), _bits(ref))
    # [B,C,H,W] form, and the whole route from the disparity
    got4 = seed.median_filter_2d(_t(_raw_depth(clip))[:, None], 11)
    assert got4.shape == (12, 1, 45, 70) and torch.equal(_bits(got4[:, 0]), _bits(ref))
    assert torch.equal(_bits(seed.depth_from_disparity(_t(clip["disp"]))), _bits(ref))
    assert torch.equal(_bits(seed.depth_from_disparity(_t(clip["disp"][7]))), _bits(ref[7]))


def _torch_median(x, k):
    x = F.pad(x[:, None], (k // 2,) * 4, mode="reflect")
    x = x.unfold(2, k, 1).unfold(3, k, 1)
    return x.contiguous().view(x.size()[:4] + (-1,)).median(dim=-1)[0][:, 0]


_SHAPES = [(6, 6), (17, 33), (45, 70)] + [(MED_TILE[0] + a, MED_TILE[1] + b) for a, b in ((-1, -1), (0, 0), (1, 1), (0, 1), (1, 0))] \
          + [(2 * MED_TILE[0] + 1, 2 * MED_TILE[1] - 1)]


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11])
def test_median_against_torch_unfold(gpu, clip, k):
    """every kernel size on the smallest legal plane, odd sizes, the fixture's size and planes one pixel either side of the
    output tile; the planes are crops of the fixture's depth, the constant frame (3) and the 8-level frame (7) included"""
    raw = _raw_depth(clip)
    for (h, w) in _SHAPES:
        x = torch.from_numpy(np.ascontiguousarray(raw[[0, 3, 7, 11], 20:20 + h, :w] if h <= 25 else raw[[0, 3, 7, 11], :h, :w]))
        assert x.shape == (4, h, w)
        got = seed.median_filter_2d(x.cuda(), k)
        assert torch.equal(_bits(got), _bits(_torch_median(x, k))), (k, h, w)


def test_median_negative_values_and_many_planes(gpu):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(70, 9, 33, generator=g)
    x[::7] = torch.round(x[::7] * 2) / 2 + 0.25          # ties, both signs (no zeros: -0 and +0 are one value to torch)
    assert torch.equal(_bits(seed.median_filter_2d(x.cuda(), 5)), _bits(_torch_median(x, 5)))


# ----------------------------------------------------------------------------------------------------------- lifting
def _fg(clip, efg):
    return (clip["masks"] == (1 if efg else -1)).astype(np.float32)


def _img(clip, frame):
    return clip["imgs"][list(clip["img_frames"]).index(frame)]


def _close(got, ref, bound, what):
    err = float((got.detach().double().cpu() - torch.from_numpy(np.asarray(ref)).double()).abs().max()) if got.numel() else 0.0
    print(f"{what}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("q", [0, 7])
@pytest.mark.parametrize("efg", [1, 0])
def test_lift_tracks_against_the_reference(gpu, clip, q, efg):
    pre = f"q{q}_fg{efg}_"
    out, valid = seed.lift_tracks(_t(clip[f"q{q}_tracks_2d"]), _t(clip["depths"]), _t(_fg(clip, efg)), q, _t(_img(clip, q)),
                                  extract_fg=bool(efg), return_valid=True)
    assert np.array_equal(valid.cpu().numpy(), clip[pre + "valid"])
    assert out.visibles.dtype == torch.bool and out.invisibles.dtype == torch.bool
    assert np.array_equal(out.visibles.cpu().numpy(), clip[pre + "visibles"])
    assert np.array_equal(out.invisibles.cpu().numpy(), clip[pre + "invisibles"])
    ref3 = clip[pre + "tracks_3d"]
    assert tuple(out.tracks_3d.shape) == ref3.shape
    _close(out.tracks_3d[..., :2], ref3[..., :2], 4 * EPS, "x, y")
    _close(out.tracks_3d[..., 2], ref3[..., 2], 8 * EPS * float(np.abs(ref3[..., 2]).max()), "depth")
    _close(out.confidences, clip[pre + "confidences"], 4e-7, "confidences")
    _close(out.colors, clip[pre + "colors"], 8 * EPS * float(np.abs(clip[pre + "colors"]).max()), "colours")


def test_normalize_depths(gpu, clip):
    d, lo, hi = seed.normalize_depths(_t(clip["depth_med"]))
    assert lo.is_cuda and hi.is_cuda and float(lo) == float(clip["depth_min"]) and float(hi) == float(clip["depth_max"])
    _close(d, clip["depths"], 4 * EPS * 2.0, "normalised depths")


def test_extend_tracks_3d_against_the_reference(gpu, clip):
    d, lo, hi = seed.normalize_depths(_t(clip["depth_med"]))
    tr = _t(clip["q0_fg1_tracks_3d"])
    T = tr.shape[1]
    masks = clip["masks"].astype(np.float32)
    pts, col = seed.extend_tracks_3d(tr, _t(clip["depth_med"][0]), _t(clip["depth_med"][T - 1]), _t(_img(clip, 0)),
                                     _t(_img(clip, T - 1)), _t(masks[0]), _t(masks[T - 1]), lo, hi,
                                     grid_size=int(clip["ext_grid_size"]), margin=float(clip["ext_margin"]))
    ref = clip["ext_points"]
    assert tuple(pts.shape) == ref.shape and tuple(col.shape) == clip["ext_colors"].shape      # identical point counts
    _close(pts[..., :2], ref[..., :2], 4 * EPS, "x, y")
    _close(pts[..., 2], ref[..., 2], 8 * EPS * float(np.abs(ref[..., 2]).max()), "depth")
    _close(col, clip["ext_colors"], 8 * EPS * float(np.abs(clip["ext_colors"]).max()), "colours")


# ------------------------------------------------------------------------------------------------------------ spline
def _walk(N, T, seed_):
    """tracks in the lifted coordinates: x, y in [-1, 1], depth in [0.5, 2], a random walk of 0.02 per frame"""
    rng = np.random.default_rng(seed_)
    start = np.concatenate([rng.uniform(-1, 1, size=(N, 1, 2)), rng.uniform(0.5, 2.0, size=(N, 1, 1))], axis=2)
    steps = 0.02 * rng.normal(size=(N, T, 3))
    steps[:, 0] = 0
    return (start + np.cumsum(steps, axis=1)).astype(np.float32)


def _assert_spline(cubic, tracks, clock, what):
    from scipy.interpolate import CubicSpline
    N, T = tracks.shape[:2]
    x = clock.intervals
    idx = seed.knot_frames(clock, T)
    I = len(x) - 1
    y = tracks[:, idx] - tracks[:, :1]                                           # float32, as the reference's delta_position
    ref = CubicSpline(x.astype(np.float64), y.astype(np.float64), axis=1).c      # [4, I, N, 3]
    ref = ref.transpose(2, 0, 1, 3).astype(np.float32).astype(np.float64)        # the reference's [N, 4, I, 3], rounded once
    got = cubic.detach().cpu().numpy().reshape(N, 4, I, 3).astype(np.float64)
    h = np.diff(x.astype(np.float64))
    ymax = float(np.abs(y).max())
    worst = 0.0
    for k in range(4):
        bound = EPS * np.abs(ref[:, k]) + 1e-10 * ymax / (h ** (3 - k))[None, :, None]
        err = np.abs(got[:, k] - ref[:, k])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), f"{what}: c[{k}] off by {float((err / np.maximum(bound, 1e-300)).max()):.2f} x the bound"
    print(f"{what}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("T", [2, 5, 6, 10, 11, 16, 50])
def test_fit_cubic_nodes_against_scipy(gpu, T):
    """2 knots (T = 2, 5), 3 knots (6, 10), the first 4- and 5-knot systems (11, 16), a generic one (50); one Gaussian, one
    short of / one past a workgroup of 64 threads per coordinate, several workgroups"""
    for N in (1, 63, 65, 257):
        tracks = _walk(N, T, 100 * T + N)
        position, cubic, clock = seed.fit_cubic_nodes(_t(tracks))
        I = clock.interval_num
        assert clock.num_frames == T and I == math.ceil(T / 5) and tuple(cubic.shape) == (N, 12 * I)
        assert np.array_equal(position.cpu().numpy(), tracks[:, 0])
        _assert_spline(cubic, tracks, clock, f"T {T} N {N}")
        # the fit interpolates: the model's own evaluation returns the track at every knot frame
        dg = DynamicGaussians(clock, position, cubic, torch.zeros(N, 4, device="cuda"), torch.zeros(N, 1, device="cuda"),
                              torch.zeros(N, 3, device="cuda"))
        for f in seed.knot_frames(clock, T):
            _close(dg.get_position(int(f)), tracks[:, f], 8 * EPS * float(np.abs(tracks).max()), f"T {T} N {N} knot frame {f}")


def test_fit_cubic_nodes_uneven_knots_and_the_fixture(gpu, clip):
    tracks = _walk(130, 40, 7)
    clock = FrameClock(40, intervals=np.array([0, 2, 3, 11, 20, 38, 39], np.float32) / np.float32(39))
    _, cubic, _ = seed.fit_cubic_nodes(_t(tracks), clock)
    _assert_spline(cubic, tracks, clock, "uneven knots")
    # the reference's own fit of the fixture's lifted tracks
    t3 = clip["q0_fg1_tracks_3d"]
    position, cubic, clock = seed.fit_cubic_nodes(_t(t3))
    assert np.array_equal(clock.intervals, clip["spline_intervals"])
    ref = clip["spline_coeff"].astype(np.float64)
    got = cubic.cpu().numpy().reshape(ref.shape).astype(np.float64)
    h = np.diff(clock.intervals.astype(np.float64))
    ymax = float(np.abs(t3 - t3[:, :1]).max())
    for k in range(4):
        assert (np.abs(got[:, k] - ref[:, k]) <= EPS * np.abs(ref[:, k]) + 1e-10 * ymax / (h ** (3 - k))[None, :, None]).all(), k
    with pytest.raises(ValueError):
        seed.fit_cubic_nodes(_t(tracks), FrameClock(40, intervals=[0.0, 0.5, 0.5, 1.0]))
    with pytest.raises(ValueError):
        seed.fit_cubic_nodes(_t(tracks), FrameClock(40, intervals=list(np.linspace(0, 1, 65))))
    with pytest.raises(ValueError):
        seed.fit_cubic_nodes(_t(tracks[:, :20]), FrameClock(40))                 # knots on frames the tracks do not have


# ----------------------------------------------------------------------------------------------------------- seeding
def _fixture_set(clip):
    t3 = np.concatenate([clip[f"q{q}_fg{e}_tracks_3d"] for q in (0, 7) for e in (1, 0)] + [clip["ext_points"]])
    col = np.concatenate([clip[f"q{q}_fg{e}_colors"] for q in (0, 7) for e in (1, 0)] + [clip["ext_colors"]])
    return t3, col


def test_seeded_set_has_the_synthetic_sets_layout(gpu, clip):
    from splatter_a_video_amd import train_step as TS
    from splatter_a_video_amd.knn import distCUDA2
    from splatter_a_video_amd.synth import make_scene
    t3, col = _fixture_set(clip)
    N, T = t3.shape[:2]
    params, clock = seed.seed_dynamic_gaussians(_t(t3), colors=_t(col), init_opacity=0.5, attrs=16)
    like = TS.synthetic_video_params(make_scene(N, 70, 45, F=T), FrameClock(T), "cuda", attrs=16)
    assert list(params) == list(like)
    for k in like:
        assert params[k].shape == like[k].shape and params[k].dtype == like[k].dtype and params[k].is_cuda, k
    assert np.array_equal(params["position"].cpu().numpy(), t3[:, 0])
    want = torch.log(torch.sqrt(torch.clamp_min(distCUDA2(params["position"]), 1e-7)))[:, None].repeat(1, 3)
    assert torch.equal(params["scaling"], want)
    assert torch.equal(params["rotation"], torch.tensor([1.0, 0, 0, 0], device="cuda").expand(N, 4))
    assert float(params["opacity"].abs().max()) == 0.0                           # logit(0.5)
    assert all(float(params[k].abs().max()) == 0.0 for k in ("rot_poly_feat", "rot_fourier_feat", "attrs"))
    assert float(params["shs"][:, 1:].abs().max()) == 0.0
    _close(params["shs"][:, 0], (col - 0.5) / 0.28209479177387814, 4 * EPS * 2.0, "SH DC")
    p2, _ = seed.seed_dynamic_gaussians(_t(t3), init_opacity=0.1, attrs=4, generator=torch.Generator(device="cuda").manual_seed(1))
    assert p2["attrs"].shape == (N, 4) and abs(float(p2["opacity"][0]) - math.log(0.1 / 0.9)) < 1e-6
    dc = p2["shs"][:, 0]
    assert float(dc.min()) >= 0.0 and float(dc.max()) <= 1.0 / 255.0 and float(dc.std()) > 0


def test_a_track_with_a_nan_is_dropped(gpu, clip):
    t3, col = _fixture_set(clip)
    bad = t3.copy()
    bad[5, 3, 1] = np.nan
    params, clock = seed.seed_dynamic_gaussians(_t(bad), colors=_t(col))
    keep = np.ones(len(t3), bool)
    keep[5] = False
    assert params["position"].shape[0] == len(t3) - 1
    assert np.array_equal(params["position"].cpu().numpy(), t3[keep, 0])
    _close(params["shs"][:, 0], (col[keep] - 0.5) / 0.28209479177387814, 4 * EPS * 2.0, "SH DC")
    assert all(bool(torch.isfinite(v).all()) for v in params.values())


def test_training_step_runs_on_the_seeded_set(gpu, clip):
    from splatter_a_video_amd import train_step as TS
    t3, col = _fixture_set(clip)
    params, clock = seed.seed_dynamic_gaussians(_t(t3), colors=_t(col))
    W, H, Fn = 70, 45, 2
    extr = torch.eye(4, device="cuda")
    t1, t2 = [0, 6], [4, 11]
    gt = TS.render_ground_truth(params, clock, W, H, extr, t1, t2)
    assert float(gt["rgb"].abs().max()) > 0                                      # the seeded Gaussians are on screen
    start = dict(params)
    start["shs"] = params["shs"] + 0.2
    start["pos_cubic_node"] = torch.zeros_like(params["pos_cubic_node"])
    st = TS.TrainingStep(start, clock, W, H, Fn, extr, K=8, arap_samples=64)
    st.step(t1, t2, gt)
    torch.cuda.synchronize()
    loss = st.loss()
    print("loss of the first step on the seeded set:", loss)
    assert np.isfinite(loss) and loss > 0
    assert bool(torch.isfinite(st.bucket.flat_grad).all()) and float(st.bucket.flat_grad.abs().max()) > 0


def test_entry_points_run_deterministically(gpu, clip):
    """no float atomics: the three entry points run under splat_set_deterministic(1), and two runs give identical bits"""
    was = L.deterministic()
    L.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            med = seed.median_filter_2d(_t(_raw_depth(clip)), 11)
            lifted = seed.lift_tracks(_t(clip["q7_tracks_2d"]), _t(clip["depths"]), _t(_fg(clip, 1)), 7, _t(_img(clip, 7)))
            position, cubic, _ = seed.fit_cubic_nodes(lifted.tracks_3d)
            runs.append([med, lifted.tracks_3d, lifted.colors, lifted.confidences, lifted.visibles.to(torch.float32),
                         position, cubic])
        torch.cuda.synchronize()
        for a, b in zip(*runs):
            assert a.numel() > 0 and torch.equal(_bits(a), _bits(b))
    finally:
        L.set_deterministic(was)
