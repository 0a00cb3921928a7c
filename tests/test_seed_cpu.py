"""Seeding stage (splatter_a_video_amd/seed.py over csrc/seed.hip), the part that needs no GPU: the entry points exist under
the unchanged ABI version, refuse bad arguments before any HIP call, return at once on empty inputs, and the Python functions
have no CPU fallback."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["splat_median_filter_2d", "splat_lift_tracks", "splat_fit_cubic_nodes"]


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def _f32(*v):
    return (ctypes.c_float * len(v))(*v)


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_symbols_exported_declared_and_listed(L):
    header = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    declared = set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", header))
    so = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SYMBOLS and hasattr(so, name), name
    assert L.lib().splat_abi_version() == 22 and L.ABI_VERSION == 22
    assert int(re.search(r"#define SPLAT_SPLINE_MAX_KNOTS (\d+)", header).group(1)) == 64
    from splatter_a_video_amd import seed
    assert seed.MAX_KNOTS == 64


def test_median_refusals_and_empty_input(L):
    lib = L.lib()
    one = ctypes.c_void_p(8)      # never dereferenced: every case returns before a launch
    med = lambda P, H, W, k: lib.splat_median_filter_2d(P, H, W, k, one, one, None)
    assert med(-1, 8, 8, 3) == -1 and b"bad sizes" in lib.splat_last_error()
    assert med(1, -8, 8, 3) == -1 and med(1, 8, -8, 3) == -1
    assert med(1, 32, 32, 4) == -1 and b"odd" in lib.splat_last_error()          # even k
    assert med(1, 32, 32, 13) == -1 and b"odd" in lib.splat_last_error()         # k > 11
    assert med(1, 32, 32, 1) == -1
    assert med(1, 5, 32, 11) == -1 and b"reflect" in lib.splat_last_error()      # H <= k // 2
    assert med(1, 32, 1, 3) == -1                                                # W <= k // 2
    assert med(0, 32, 32, 11) == 0                                               # P = 0: nothing to do, no launch
    assert lib.splat_median_filter_2d(1, 32, 32, 11, None, None, None) == -1 and b"null" in lib.splat_last_error()


def test_lift_refusals_and_empty_input(L):
    lib = L.lib()
    one = ctypes.c_void_p(8)
    lift = lambda N, T, H, W, q: lib.splat_lift_tracks(N, T, H, W, one, one, one, q, one, 0, one, one, one, one, one, one, one, None)
    assert lift(-1, 4, 8, 8, 0) == -1 and b"bad sizes" in lib.splat_last_error()
    assert lift(4, 4, -8, 8, 0) == -1
    assert lift(4, 4, 8, 8, 4) == -1 and b"query_index" in lib.splat_last_error()
    assert lift(4, 4, 8, 8, -1) == -1
    assert lift(0, 4, 8, 8, 0) == 0                                              # N = 0
    assert lift(4, 0, 8, 8, 0) == 0 and lift(4, 4, 0, 8, 0) == 0 and lift(4, 4, 8, 0, 0) == 0   # T * H * W = 0


def test_spline_refusals_and_empty_input(L):
    lib = L.lib()
    one = ctypes.c_void_p(8)
    fit = lambda N, T, knots, frames: lib.splat_fit_cubic_nodes(N, T, len(knots), _f32(*knots), _i32(*frames), one, one, one, None)
    assert fit(-1, 4, [0.0, 1.0], [0, 3]) == -1 and b"bad sizes" in lib.splat_last_error()
    assert fit(4, 4, [0.0], [0]) == -1 and b"at least 2" in lib.splat_last_error()             # fewer than 2 knots
    assert fit(4, 9, [0.0, 0.5, 0.5, 1.0], [0, 4, 4, 8]) == -1 and b"increasing" in lib.splat_last_error()
    assert fit(4, 9, [0.0, 0.6, 0.5, 1.0], [0, 5, 4, 8]) == -1 and b"increasing" in lib.splat_last_error()
    assert fit(4, 4, [0.0, 1.0], [0, 4]) == -1 and b"outside the clip" in lib.splat_last_error()   # knot frame >= T
    many = np.linspace(0.0, 1.0, 65)
    assert fit(4, 100, list(many), list(range(65))) == -1 and b"MAX_KNOTS" in lib.splat_last_error()
    assert lib.splat_fit_cubic_nodes(4, 4, 2, None, None, one, one, one, None) == -1
    assert fit(0, 4, [0.0, 1.0], [0, 3]) == 0                                    # N = 0: no launch
    assert fit(0, 64, list(np.linspace(0.0, 1.0, 64)), list(range(64))) == 0     # the cap itself is accepted


def test_python_functions_refuse_cpu_tensors_and_wrong_shapes(L):
    from splatter_a_video_amd import seed
    z = torch.zeros
    with pytest.raises(ValueError):
        seed.median_filter_2d(z(1, 1, 16, 16))
    with pytest.raises(ValueError):
        seed.median_filter_2d(z(16, 16))                                          # neither [B,C,H,W] nor [T,H,W]
    with pytest.raises(ValueError):
        seed.median_filter_2d(z(1, 16, 16), kernel_size=4)
    with pytest.raises(ValueError):
        seed.median_filter_2d(z(1, 16, 16), kernel_size=13)
    with pytest.raises(ValueError):
        seed.depth_from_disparity(z(16, 16))
    with pytest.raises(ValueError):
        seed.normalize_depths(z(2, 16, 16))
    with pytest.raises(ValueError):
        seed.lift_tracks(z(5, 4, 4), z(4, 8, 8), z(4, 8, 8), 0, z(8, 8, 3))
    with pytest.raises(ValueError):
        seed.extend_tracks_3d(z(5, 4, 3), z(8, 8), z(8, 8), z(8, 8, 3), z(8, 8, 3), z(8, 8), z(8, 8), z(()), z(()))
    with pytest.raises(ValueError):
        seed.fit_cubic_nodes(z(5, 4, 3))
    with pytest.raises(ValueError):
        seed.seed_dynamic_gaussians(z(5, 4, 3))
    assert seed.LiftedTracks._fields == ("tracks_3d", "colors", "visibles", "invisibles", "confidences")


def test_knot_frames_are_the_references(L):
    """round(intervals * (T - 1)) gives back the truncated-linspace frame indices the default clock was built from"""
    from splatter_a_video_amd import seed
    from splatter_a_video_amd.dynamics import FrameClock
    for T in (2, 5, 6, 10, 11, 12, 16, 50, 100, 313):
        idx = torch.linspace(0, T - 1, -(-T // 5) + 1).long().numpy()
        assert np.array_equal(seed.knot_frames(FrameClock(T), T), idx), T
