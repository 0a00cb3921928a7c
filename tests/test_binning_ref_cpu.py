"""tests/binning_ref.py (the numpy reference of tile binning + sort) against the C oracle's sort_gaussian, bit for bit, on every
case the GPU tests use -- and the constants of csrc/binning.hip the case list is built around, parsed out of the source: a
retuned constant fails here instead of silently moving a case off the branch its name promises."""
import os
import re

import numpy as np
import pytest

import binning_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _oracle_sort(o, uv, depth, radius, W, H):
    x0, y0, x1, y1 = R.rect(uv, radius, W, H)      # `tiles` only sizes the oracle's arrays; its keys come from its own tile_rect
    idx, tr = o.sort_gaussian(uv, depth, W, H, radius, ((x1 - x0) * (y1 - y0)).astype(np.int32))
    return idx, tr


def _check(o, uv, depth, radius, W, H, ref):
    idx, tr = _oracle_sort(o, uv, depth, radius, W, H)
    assert ref.M == idx.size == int(ref.gcount.sum())
    assert np.array_equal(ref.idx_sorted, idx)
    assert np.array_equal(ref.tile_range, tr)
    # the slots: a permutation whose entries name their owner, ascending inside every Gaussian along its row-major rectangle
    assert np.array_equal(np.sort(ref.slot_sorted), np.arange(ref.M))
    owner = np.repeat(np.arange(radius.size), ref.gcount)
    assert np.array_equal(owner[ref.slot_sorted], ref.idx_sorted)
    assert np.array_equal(ref.goff_incl, np.cumsum(ref.gcount))


def test_source_constants():
    src = open(os.path.join(ROOT, "splatter_a_video_amd", "csrc", "binning.hip")).read()
    d = lambda name: int(re.search(r"^#define %s (\d+)\b" % name, src, re.M).group(1))
    for name in ("BIN_BLOCK", "BIN_MAX_NB", "BIN_CHUNK", "BIN_CHUNK_BATCH", "BIN_BATCH_FRAMES", "BIN_LDS_TILES", "BIN_GLOBAL_BLOCKS",
                 "SORT_BLOCK", "COLSCAN_COLS"):
        assert d(name) == getattr(R, name), name
    assert re.search(r"^#define COLSCAN_GROUPS \(1024 / COLSCAN_COLS\)", src, re.M) and R.COLSCAN_GROUPS == 1024 // R.COLSCAN_COLS
    # the tile scan: one workgroup of 1024 threads striding by 1024 over the tiles and over the chunks
    assert re.search(r"__launch_bounds__\((\d+)\)\s*bin_tilescan_kernel", src).group(1) == str(R.TILESCAN_THREADS)
    assert re.search(r"bin_tilescan_kernel, dim3\(1, F\), dim3\((\d+)\)", src).group(1) == str(R.TILESCAN_THREADS)
    assert len(re.findall(r"base \+= 1024\)", src)) == 2 and len(re.findall(r"threadIdx\.x == 1023", src)) == 2
    # the size classes of the per-tile sort: 2, 4 and 8 keys per thread, above that the crowded path
    for r in (2, 4, 8):
        assert "n <= %d * SORT_BLOCK" % r in src


def test_case_names_keep_their_promise():
    """the branch facts every plan case is there for, from the constants pinned above"""
    p = {c.name: R.plan(c.P, c.W, c.H) for c in R.PLAN_CASES}
    assert [c.T for c in R.PLAN_CASES] == [1, 1, 1023, 1024, 1025, 819, 1025, 12288, 12288, 12288, 12288, 1024, 12288,
                                           12289, 12289, 12319, 12319, 12289, 12319]
    assert all(v["lds"] == (v["T"] <= 12288) for v in p.values())
    assert sorted({c.T for c in R.PLAN_CASES if not p[c.name]["lds"]}) == [12289, 12319]
    assert {c.P for c in R.PLAN_CASES if p[c.name]["lds"]} == {1, 255, 256, 257, 512, 513, 16385, 262144, 262145}
    assert {c.P for c in R.PLAN_CASES if not p[c.name]["lds"]} == {1, 257, 5000, 262145, 524800}
    assert p["T1025_P512"]["NB"] == 1 and p["T819odd_P513"]["NB"] == 2 and p["T819odd_P513"]["chunk"] == 257
    assert p["T1025_P16385"]["NB"] == 33 and p["T1025_P16385"]["rpg"] == 2 and p["T12288x1_P16385"]["rpg"] == 2
    assert p["T6144x2_P262144"]["NB"] == 512 and p["T6144x2_P262144"]["chunk"] == 512 and p["T6144x2_P262144"]["rpg"] == 16
    assert p["T1024_P262145"]["NB"] == 512 and p["T1024_P262145"]["chunk"] == 513 and p["T1024_P262145"]["packed"]
    assert p["T12288x1_P262145"]["chunk"] == 513 and not p["T12288x1_P262145"]["packed"]
    assert p["T6144x2_P262144"]["packed"]
    assert p["T12289x1_P257"]["nchunk"] == 2 and p["T12289x1_P257"]["chunk"] == 129
    assert p["T12289x1_P262145"]["nchunk"] == 1025 > R.TILESCAN_THREADS
    assert p["T97x127_P524800"]["nchunk"] == R.BIN_GLOBAL_BLOCKS and p["T97x127_P524800"]["chunk"] == 257 > R.BIN_BLOCK
    w = [c for c in R.PLAN_CASES if c.W % 16 and c.H % 16]
    assert len(w) >= 2 and all(c.branch for c in R.PLAN_CASES) and len(p) == len(R.PLAN_CASES)
    # frame batch: BIN_CHUNK_BATCH chunks from BIN_BATCH_FRAMES frames on
    assert [R.plan(P, 320, 240, 4)["NB"] for P in (2047, 2048, 2049, 5000)] == [1, 1, 2, 3]
    assert [R.plan(P, 320, 240, 3)["NB"] for P in (2047, 2048, 2049, 5000)] == [4, 4, 5, 10]


@pytest.mark.parametrize("case", R.PLAN_CASES, ids=lambda c: c.name)
def test_plan_cases_equal_the_oracle(oracle_mod, case):
    uv, depth, radius = R.case_inputs(case)
    ref = R.case_reference(case.name)
    _check(oracle_mod, uv, depth, radius, case.W, case.H, ref)
    assert 0 < ref.M < 1_100_000
    if 256 <= case.P <= 20000:
        assert int(ref.gcount.max()) == case.T           # one rectangle is the whole grid
    if case.P >= 256:
        assert (radius <= 0).any() and (ref.gcount[radius > 0] == 0).any()      # dead radii, and live ones off the image


@pytest.mark.parametrize("pattern", R.DEPTH_PATTERNS)
def test_length_cases_equal_the_oracle(oracle_mod, pattern):
    uv, depth, radius, W, H, tile = R.length_inputs(pattern)
    ref = R.length_reference(pattern)
    _check(oracle_mod, uv, depth, radius, W, H, ref)
    assert (ref.tile_range[:, 1] - ref.tile_range[:, 0]).tolist() == R.LIST_LENGTHS
    if pattern in ("equal",):       # bit-equal depths: ascending id inside every tile
        assert np.array_equal(ref.idx_sorted, np.argsort(tile, kind="stable"))


@pytest.mark.parametrize("W,H", [(77, 50), (16 * 12289, 16)])
def test_edge_cases_equal_the_oracle(oracle_mod, W, H):
    uv, depth, radius = R.edge_inputs(W, H)
    ref = R.sort(uv, depth, radius, W, H)
    _check(oracle_mod, uv, depth, radius, W, H, ref)
    gx, gy = R.grid(W, H)
    assert int((ref.gcount == gx * gy).sum()) == 3 and int(((radius > 0) & (ref.gcount == 0)).sum()) >= 6
    # the reference-flow keys: the oracle's compute_gaussian_key on the same inputs
    key, gid = R.keys(uv, depth, radius, W, H)
    okey, oidx = oracle_mod.compute_gaussian_key(uv, depth, W, H, radius, ref.goff_incl)
    assert np.array_equal(key, okey) and np.array_equal(gid, oidx)


def test_rect_truncates_toward_zero_and_clamps():
    f = np.float32
    uv = np.array([[-3, 4], [15.5, 16], [16, 31.99], [1e6, -1e6], [40, 40], [40, 40]], f)
    r = np.array([5, 1, 1, 3, 0, -4], np.int32)
    x0, y0, x1, y1 = R.rect(uv, r, 64, 48)
    assert x0.tolist() == [0, 0, 0, 4, 0, 0] and x1.tolist() == [1, 1, 2, 4, 0, 0]
    assert y0.tolist() == [0, 0, 1, 0, 0, 0] and y1.tolist() == [1, 2, 2, 0, 0, 0]
    with pytest.raises(AssertionError):
        R.depth_bits(np.array([-1.0], f))
    with pytest.raises(AssertionError):
        R.depth_bits(np.array([np.nan], f))
