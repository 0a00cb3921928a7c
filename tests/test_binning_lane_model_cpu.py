"""tools/binning_lane_model.py on a scene of a few thousand Gaussians: the order it models for the kernels visits every Gaussian
with tiles of every chunk exactly once, its constants are those of csrc/binning.hip, and it never runs more trips per wave than
the stored order."""
import os
import re
import sys

import numpy as np
import pytest

import binning_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import binning_lane_model as M  # noqa: E402

W, H, P = 320, 240, 5000


@pytest.fixture(scope="module")
def area():
    uv, _, radius = R.random_inputs(P, W, H, 40, 99)
    rng = np.random.default_rng(5)
    radius[rng.random(P) < 0.5] = 3                 # many small rectangles beside the large ones, as in a real scene
    x0, y0, x1, y1 = R.rect(uv, radius, W, H)
    a = ((x1 - x0) * (y1 - y0)).astype(np.int64)
    assert (a == 0).any() and (a >= 32).any() and (a == 1).any()
    assert ((a > M.BIN_INLINE_AREA) & (a < M.BIN_BIG_AREA)).any() and (a == M.BIN_INLINE_AREA).any() and (a == M.BIN_BIG_AREA).any()
    return a


def test_constants_are_those_of_the_kernels():
    src = open(os.path.join(ROOT, "splatter_a_video_amd", "csrc", "binning.hip")).read()
    for name in ("BIN_SEG", "BIN_INLINE_AREA", "BIN_BIG_AREA"):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == getattr(M, name), name
    assert re.search(r"const bool defer = area > BIN_INLINE_AREA;\s*defer_append\(defer, area >= BIN_BIG_AREA,", src)
    assert re.search(r"const bool defer = walk > BIN_INLINE_AREA;\s*defer_append\(defer, walk >= BIN_BIG_AREA,", src)
    c = M.area_class(np.arange(0, 200))
    assert c[0] == 9 and c[1] == 8 and c[2] == 7 and c[4] == 6 and c[5] == 5 and c[31] == 1 and c[32] == 0 and (np.diff(c) <= 0).all()


@pytest.mark.parametrize("chunk", [2041, 586, 257, 64, 1])
@pytest.mark.parametrize("seg", [M.BIN_SEG, 256])
def test_every_gaussian_of_every_chunk_once(area, chunk, seg):
    for beg, end in M.chunks(P, chunk):
        a = area[beg:end]
        v = M.visits(area, beg, end, seg)
        assert np.array_equal(np.sort(v), np.arange(end - beg))                      # a permutation of the chunk
        passes = M.order_built(area, beg, end, seg)
        assert len(passes) == 2 * -(-(end - beg) // seg)
        for s, (stored, deferred) in enumerate(zip(passes[0::2], passes[1::2])):
            lo, hi = s * seg, min(end - beg, (s + 1) * seg)
            assert np.array_equal(stored[0], np.arange(lo, hi)) and np.array_equal(stored[1], a[lo:hi] <= M.BIN_INLINE_AREA)
            d = deferred[0]
            assert deferred[1].all() and ((d >= lo) & (d < hi)).all() and (a[d] > M.BIN_INLINE_AREA).all()
            assert (np.diff((a[d] >= M.BIN_BIG_AREA).astype(int)) <= 0).all()        # the large rectangles lead the list


@pytest.mark.parametrize("chunk", [2041, 586, 257])
def test_built_order_never_runs_more_trips(area, chunk):
    for beg, end in M.chunks(P, chunk):
        stored = M.wave_trips(area, beg, M.order_stored(area, beg, end))
        built = M.wave_trips(area, beg, M.order_built(area, beg, end))
        exact = M.wave_trips(area, beg, M.order_area(area, beg, end))
        assert exact <= built <= stored, (beg, exact, built, stored)
    m = M.model(area, chunk)
    assert m["built"]["trips_per_64_gaussians"] <= m["stored"]["trips_per_64_gaussians"]
    assert m["stored"]["lane_utilisation"] <= m["built"]["lane_utilisation"] <= m["area"]["lane_utilisation"] <= 1.0
