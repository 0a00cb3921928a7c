"""Point tracking without a GPU: the float64 sampling reference (tests/track_query_ref.py) against torch's grid_sample, the
documented sampling position against the reference's normalize_coords + align_corners=True chain, the two new C ABI entries
(csrc/query.hip) exported, declared and refusing bad arguments with SPLAT_E_ARG before any HIP call, and the Python operators
refusing what they cannot serve."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import track_query_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["splat_alpha_blending_points_forward", "splat_track_flow_rows"]


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def _points(rng, W, H, n=200):
    """random points + the places a sampler goes wrong: integers, the image border, half outside, fully outside, not finite"""
    p = [rng.uniform(-2, [W + 1, H + 1], size=(n, 2)),
         np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.float64),
         np.round(rng.uniform(0, [W - 1, H - 1], size=(n, 2)) * 8) / 8,
         [[0, 0], [W - 1, H - 1], [W - 1, 0], [0, H - 1], [W - 1.5, H - 1.5], [W - 1, 3.25], [2.5, H - 1]],
         [[-0.5, 3], [3, -0.5], [W - 0.5, 3], [3, H - 0.75], [-0.25, -0.25], [W - 0.5, H - 0.5], [-1, 2], [W, 2], [2, H]],
         [[-1.001, 2], [-7, -7], [W + 0.01, 2], [2, H + 3], [1e9, 1e9], [-1e9, 4], [3, 1e30]]]
    return np.concatenate([np.asarray(a, np.float64) for a in p]).astype(np.float32)


@pytest.mark.parametrize("C,H,W", [(1, 5, 7), (3, 48, 64), (4, 1, 9), (2, 6, 1)])
def test_sample_points_is_grid_sample(C, H, W):
    rng = np.random.default_rng(C * 100 + W)
    img = rng.normal(size=(C, H, W))
    pts = _points(rng, W, H)
    got = R.sample_points(img, pts)
    # grid_sample in float64 on the normalised grid of align_corners=True: x_n = 2 ix / (W - 1) - 1 (a one-pixel axis cannot be
    # normalised: its rows are checked against the definition below instead)
    if W > 1 and H > 1:
        p64 = torch.from_numpy(pts.astype(np.float64))
        grid = torch.stack([2 * p64[:, 0] / (W - 1) - 1, 2 * p64[:, 1] / (H - 1) - 1], -1)
        want = F.grid_sample(torch.from_numpy(img)[None], grid[None, :, None, :], mode="bilinear", padding_mode="zeros",
                             align_corners=True)[0, :, :, 0].T.numpy()
        # (the normalisation and its inverse round: an exact-integer coordinate may come back 1e-16 off, which moves weight
        # between two corners by that much)
        tol = 1e-9 * (1 + np.abs(img).max())
        far = np.abs(pts).max(1) > 1e6           # beyond float64's grid resolution torch's own index arithmetic is not exact
        assert np.abs(got - want)[~far].max() < tol
        assert (got[far] == 0).all() and far.sum() >= 3
    # the definition, point by point
    for q in range(0, pts.shape[0], 7):
        ix, iy = float(pts[q, 0]), float(pts[q, 1])
        x0, y0 = np.floor(ix), np.floor(iy)
        want = np.zeros(C)
        for cx, cy, w in ((x0, y0, (x0 + 1 - ix) * (y0 + 1 - iy)), (x0 + 1, y0, (ix - x0) * (y0 + 1 - iy)),
                          (x0, y0 + 1, (x0 + 1 - ix) * (iy - y0)), (x0 + 1, y0 + 1, (ix - x0) * (iy - y0))):
            if 0 <= cx <= W - 1 and 0 <= cy <= H - 1:
                want += w * img[:, int(cy), int(cx)]
        np.testing.assert_allclose(got[q], want, rtol=0, atol=1e-12)


def test_sample_points_edge_semantics():
    img = np.arange(2 * 4 * 6, dtype=np.float64).reshape(2, 4, 6) + 1
    f = lambda *p: R.sample_points(img, np.array([p], np.float32))[0]
    assert (f(2, 3) == img[:, 3, 2]).all()                        # an integer lands on a stored pixel
    assert (f(5, 3) == img[:, 3, 5]).all()                        # (W - 1, H - 1): the corners past the border weigh 0
    assert (f(-0.5, 0) == 0.5 * img[:, 0, 0]).all()               # half outside: the outside corners contribute nothing
    assert (f(5.25, 1) == 0.75 * img[:, 1, 5]).all()
    assert (f(-1, 2) == 0).all() and (f(6, 2) == 0).all() and (f(2, 4) == 0).all()
    for bad in (float("nan"), float("inf"), -float("inf"), 1e9):
        assert (f(bad, 1) == 0).all() and (f(1, bad) == 0).all()
    xi, yi, inside = R.corner_pixels(np.array([[4.5, -0.5], [np.nan, 1]], np.float32), 6, 4)
    assert inside.tolist() == [[False, False, True, True], [False] * 4]
    assert (xi[0, 2:].tolist(), yi[0, 2:].tolist()) == ([4, 5], [0, 0])


@pytest.mark.parametrize("W,H", [(64, 48), (854, 480), (100, 60), (1920, 1080)])
def test_documented_sampling_position_is_the_reference_chain(W, H):
    """normalize_coords (src/util.py:65-72: coords / (w, h) * 2 - 1) followed by grid_sample's align_corners=True un-normalisation
    ((x + 1) / 2 * (size - 1)), both in float32, against ix = px * float32((W - 1) / W): within 2^-22 W"""
    from splatter_a_video_amd.tracking import sample_coords
    rng = np.random.default_rng(W)
    px = torch.from_numpy(np.concatenate([rng.uniform(0, [W, H], size=(4000, 2)),
                                          np.stack([np.arange(0, W + 1) % (W + 1), np.arange(0, W + 1) % (H + 1)], 1),
                                          [[0, 0], [W, H], [W - 1, H - 1], [0.5, 0.5]]]).astype(np.float32))
    size = torch.tensor([W, H], dtype=torch.float32)
    normed = px / size * 2 - 1.0
    chain = (normed + 1) / 2 * (size - 1)
    got = sample_coords(px, W, H)
    assert got.dtype == torch.float32
    s = np.array([np.float32((W - 1) / W), np.float32((H - 1) / H)], np.float32)
    assert np.array_equal(got.numpy(), px.numpy() * s)             # the formula itself: one float32 multiply
    err = (got.double() - chain.double()).abs()
    assert float(err[:, 0].max()) <= 2.0 ** -22 * W and float(err[:, 1].max()) <= 2.0 ** -22 * H


def test_symbols_are_exported_declared_and_the_abi_version_stays(L):
    so = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    declared = set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(so, name) and name in declared, name
    assert L.lib().splat_abi_version() == 22 and L.ABI_VERSION == 22
    assert re.search(r"#define SPLAT_ABI_VERSION 22\b", header)


def test_points_entry_validates_before_hip(L):
    lib = L.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: every call below is refused on the host
    f = ctypes.c_float

    def call(P=10, C=3, uv=one, conic=one, op=one, feat=one, idx=one, tr=one, bg=0.0, W=64, H=48, Q=5, pts=one, out=one):
        return lib.splat_alpha_blending_points_forward(P, C, uv, conic, op, feat, idx, tr, f(bg), W, H, Q, pts, out, None, None, None)
    assert call(P=-1) == -1 and b"sizes" in lib.splat_last_error()
    assert call(C=0) == -1 and call(W=0) == -1 and call(H=-2) == -1 and call(Q=-1) == -1
    assert call(W=(1 << 24) + 1) == -1 and b"too large" in lib.splat_last_error()
    assert call(pts=None) == -1 and b"null" in lib.splat_last_error()
    assert call(out=None) == -1
    assert call(uv=None) == -1 and call(conic=None) == -1 and call(op=None) == -1 and call(feat=None) == -1 and call(tr=None) == -1
    # nothing to do: valid without any pointer
    assert call(Q=0, pts=None, out=None, uv=None, conic=None, op=None, feat=None, idx=None, tr=None) == 0


def test_rows_entry_validates_before_hip(L):
    lib = L.lib()
    one = ctypes.c_void_p(16)
    f = ctypes.c_float

    def call(T=4, P=10, I=2, tab=one, pos=one, cub=one, layout=0, extr=one, W=64, H=48, near=0.01, ext=1.3, uv=one, rows=one):
        return lib.splat_track_flow_rows(T, P, I, tab, pos, cub, layout, extr, W, H, f(near), f(ext), uv, rows, None)
    assert call(T=-1) == -1 and b"sizes" in lib.splat_last_error()
    assert call(P=-1) == -1 and call(I=0) == -1 and call(W=0) == -1 and call(H=0) == -1
    assert call(layout=2) == -1 and b"cubic_layout" in lib.splat_last_error()
    assert call(near=float("nan")) == -1 and call(ext=float("nan")) == -1
    assert call(tab=None) == -1 and b"null" in lib.splat_last_error()
    for k in ("pos", "cub", "extr", "uv", "rows"):
        assert call(**{k: None}) == -1, k
    assert call(T=0, tab=None, rows=None) == 0 and call(P=0, pos=None, cub=None, uv=None, rows=None) == 0


def test_python_operators_refuse_what_they_cannot_serve(L):
    import dptr.gs as gs
    from splatter_a_video_amd import gs as native
    from splatter_a_video_amd.dynamics import FrameClock
    from splatter_a_video_amd.tracking import track_pixels
    assert gs.alpha_blending_points is native.alpha_blending_points
    z = lambda *s, **k: torch.zeros(*s, **k)
    args = lambda **k: dict(dict(uv=z(4, 2), conic=z(4, 3), opacity=z(4, 1), feature=z(4, 3), idx_sorted=z(0, dtype=torch.int32),
                                 tile_range=z(4, 2, dtype=torch.int32), bg=0.0, W=32, H=32, points=z(5, 2)), **k)
    with pytest.raises(ValueError, match="CUDA"):
        gs.alpha_blending_points(**args())                           # no CPU fallback
    with pytest.raises(ValueError, match="forward only"):
        gs.alpha_blending_points(**args(feature=z(4, 3, requires_grad=True)))
    with pytest.raises(ValueError, match="forward only"):
        gs.alpha_blending_points(**args(points=z(5, 2, requires_grad=True)))
    p = dict(position=z(4, 3), pos_cubic_node=z(4, 24), rotation=z(4, 4), rot_poly_feat=z(4, 4, 4), rot_fourier_feat=z(4, 8, 4),
             opacity=z(4, 1), scaling=z(4, 3))
    with pytest.raises(ValueError):
        track_pixels(p, FrameClock(10), 0, z(3, 2), [1, 2], torch.eye(4), 32, 32)
