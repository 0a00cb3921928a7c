"""The area order of bin_count / bin_scatter (csrc/binning.hip: a lane walks a small rectangle where it meets it and defers a
larger one to a list the workgroup walks afterwards) leaves every output where it was: binning + sort against
tests/binning_ref.py, bit for bit, on the shapes at which it can go wrong -- fewer Gaussians than a wave, chunks that are no
multiple of the workgroup, waves of one area class, chunks with every class (areas on both sides of BIN_INLINE_AREA and
BIN_BIG_AREA), a chunk whose every Gaussian is deferred, chunks of several list segments (library option
"bin_short_segments": segments of 256 instead of 2048), the global-atomic path, one hot tile counter -- with reach masks on and
off, packed keys and slot keys, one frame and five (the batch plan's larger chunks).  Every case runs with both segment lengths
and twice; all four runs must be equal.

Reach masks: binning_ref has no cull test, so the reach WORDS are checked where the decision is clear (opacity below 1/255: no
tile; a conic flat over the whole rectangle at opacity 1: every tile), must not depend on segment length or run, and everything
else (counts, prefix, tile ranges, sorted ids and slots, owner) is derived from the words in numpy and compared exactly."""
import functools

import numpy as np
import pytest
import torch

import binning_ref as R
import splatter_a_video_amd._lib as L

pytestmark = pytest.mark.gpu

SENT = -7
REACH_BIG = 1 << 31
W0, H0 = 320, 240                    # 20 x 15 tiles: LDS path
WG, HG = 16 * 97, 16 * 127           # 12319 tiles: the global-atomic path, in two dimensions
CLASS_LOWER = [32, 17, 13, 10, 7, 5, 3, 2, 1]     # area classes the cases are built from (lower bounds, largest first)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _n(t):
    return t.detach().cpu().numpy()


def _full(n, dtype=torch.int32):
    return torch.full((int(n),), SENT, dtype=dtype, device="cuda")


# ================================================================== inputs
def _conic_opacity(P, radius, seed):
    """a third each: opacity 0.003 (no tile), a flat conic at opacity 1 (every tile), an anisotropic splat of about the radius"""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, P)
    s1 = np.maximum(radius, 1) / 3.0
    s2 = s1 * rng.uniform(0.1, 1.0, P)
    th = rng.uniform(0.0, np.pi, P)
    c, s = np.cos(th), np.sin(th)
    a, b, d = c * c * s1 ** 2 + s * s * s2 ** 2, c * s * (s1 ** 2 - s2 ** 2), s * s * s1 ** 2 + c * c * s2 ** 2
    det = a * d - b * b
    conic = np.stack([d / det, -b / det, a / det], axis=1).astype(np.float32)
    opacity = rng.uniform(0.05, 0.99, P).astype(np.float32)
    conic[kind == 1] = (1e-6, 0.0, 1e-6)
    conic[(kind == 1) & (rng.random(P) < 0.3)] = 0.0          # degenerate conic: always kept
    opacity[kind == 1] = 1.0
    opacity[kind == 0] = 0.003
    return conic, opacity


def _random(P, W, H, rmax, seed):
    uv, depth, radius = R.random_inputs(P, W, H, rmax, seed)
    uv[0], radius[0] = (W / 3, H / 2), rmax          # (the only Gaussian of P = 1 has tiles)
    return uv, depth, radius


def _by_class(counts, W, H, seed, n_dead=0, shuffle=True):
    """Gaussians picked by the class of their rectangle area: counts[c] of class c (CLASS_LOWER), then n_dead without tiles (half
    radius 0, half a rectangle clipped away at the image border)"""
    rng = np.random.default_rng(seed)
    N = 60000
    uv = np.stack([rng.uniform(-20.0, W + 20.0, N), rng.uniform(-20.0, H + 20.0, N)], axis=1).astype(np.float32)
    radius = rng.integers(1, 70, N).astype(np.int32)
    radius[: N // 2] = rng.integers(1, 12, N // 2)
    x0, y0, x1, y1 = R.rect(uv, radius, W, H)
    area = (x1 - x0) * (y1 - y0)
    pick = []
    for c, n in enumerate(counts):
        lo, hi = CLASS_LOWER[c], (CLASS_LOWER[c - 1] if c else 1 << 30)
        idx = np.flatnonzero((area >= lo) & (area < hi))
        assert idx.size >= n, (c, idx.size, n)
        pick.append(idx[:n])
    pick = np.concatenate(pick)
    uv, radius = uv[pick], radius[pick]
    if n_dead:
        k = n_dead // 2
        duv = np.stack([rng.uniform(0.0, W, n_dead), rng.uniform(0.0, H, n_dead)], axis=1).astype(np.float32)
        dr = np.zeros(n_dead, np.int32)
        dr[:k // 2] = -3
        duv[k:, 0] = np.where(rng.random(n_dead - k) < 0.5, -40.0, W + 60.0)      # radius 5: clipped to nothing
        dr[k:] = 5
        uv, radius = np.concatenate([uv, duv]), np.concatenate([radius, dr])
    P = radius.size
    depth = rng.uniform(0.1, 20.0, P).astype(np.float32)
    depth[::5] = 1.5
    if shuffle:
        o = rng.permutation(P)
        uv, depth, radius = uv[o], depth[o], radius[o]
    return uv, depth, radius


def _one_tile(P, seed):
    """every Gaussian on tile (7, 4): one hot counter, lists of P entries with ties"""
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(16 * 7 + 5.0, 16 * 7 + 11.0, P), rng.uniform(16 * 4 + 5.0, 16 * 4 + 11.0, P)], axis=1).astype(np.float32)
    radius = rng.integers(1, 5, P).astype(np.int32)
    depth = rng.uniform(0.1, 9.0, P).astype(np.float32)
    depth[::3] = 2.0
    return uv, depth, radius


# name -> (W, H, builder).  F = 1 plan: chunks of at most 512; F = 5 (batch plan): chunks of at most 2048.
CASES = {
    "P1": (W0, H0, lambda: _random(1, W0, H0, 40, 1)),
    "P63": (W0, H0, lambda: _random(63, W0, H0, 40, 2)),                     # fewer Gaussians than one wave in the only chunk
    "P64": (W0, H0, lambda: _random(64, W0, H0, 40, 3)),
    "P65": (W0, H0, lambda: _random(65, W0, H0, 40, 4)),
    "P257": (W0, H0, lambda: _random(257, W0, H0, 40, 5)),                   # a chunk of 257: one Gaussian in the second trip
    "P1300_random_order": (W0, H0, lambda: _random(1300, W0, H0, 60, 6)),    # F = 1: chunks of 434; F = 5: one chunk of 1300, short
                                                                             # segments: five of 256 and one of 20 (below a wave)
    # whole waves of one-tile splats (and a deferred list of 20 rectangles of 32 tiles and more), beside radius 0 and clipped
    # rectangles, in random order
    "one_class_waves": (W0, H0, lambda: _by_class([20, 0, 0, 0, 0, 0, 0, 0, 200], W0, H0, 7, n_dead=36)),
    # the same, in stored order: Gaussians 0 .. 19 large, 20 .. 219 one tile, then the dead ones
    "one_class_waves_stored": (W0, H0, lambda: _by_class([20, 0, 0, 0, 0, 0, 0, 0, 200], W0, H0, 8, n_dead=36, shuffle=False)),
    "every_class": (W0, H0, lambda: _by_class([12, 30, 30, 40, 50, 60, 70, 70, 80], W0, H0, 9, n_dead=70)),   # 512: one chunk
    "every_class_2049": (W0, H0, lambda: _by_class([40, 100, 120, 150, 200, 250, 300, 300, 389], W0, H0, 10, n_dead=200)),
    "all_deferred": (W0, H0, lambda: _by_class([100, 100, 100, 100, 56, 56, 0, 0, 0], W0, H0, 14)),         # 512: a full list
    "one_tile": (W0, H0, lambda: _one_tile(600, 11)),
    "global_P5": (WG, HG, lambda: _by_class([1, 0, 0, 0, 0, 1, 0, 1, 1], WG, HG, 12, n_dead=1)),
    "global_P257": (WG, HG, lambda: _random(257, WG, HG, 120, 13)),
}


@functools.lru_cache(maxsize=None)
def _frames(name, F):
    """F frames of a case: frame f holds the case's Gaussians rolled by 37 f (opacity is shared by the frames and stays)"""
    W, H, build = CASES[name]
    uv, depth, radius = build()
    conic, opacity = _conic_opacity(radius.size, radius, len(name))
    return [tuple(np.roll(a, 37 * f, axis=0) for a in (uv, depth, radius, conic)) for f in range(F)], opacity


# ================================================================== reference
def _cells(w, h):
    """(log2 of the cell edge, cells per row) of the large rectangles (reach_cell_shift, csrc/binning.hip)"""
    sh = np.ones_like(w)
    for _ in range(16):
        over = (((w - 1) >> sh) + 1) * (((h - 1) >> sh) + 1) > 31
        sh = sh + over
    return sh, ((w - 1) >> sh) + 1, ((h - 1) >> sh) + 1


def _expected_words(uv, radius, conic, opacity, W, H):
    """(word, known): the reach word where the decision is clear"""
    x0, y0, x1, y1 = R.rect(uv, radius, W, H)
    w, h = x1 - x0, y1 - y0
    area = w * h
    big = area >= 32
    sh, ncx, ncy = _cells(np.maximum(w, 1), np.maximum(h, 1))
    nbits = np.where(big, ncx * ncy, area)
    none = opacity < 1.0 / 255.0
    flat = (opacity == 1.0) & (conic[:, 0] <= 1e-6)
    word = np.where(flat, (np.int64(1) << nbits) - 1, 0) | np.where(big, REACH_BIG, 0)
    word[area == 0] = 0
    return word.astype(np.uint32), none | flat | (area == 0)


def _reference(uv, depth, radius, W, H, words=None):
    """binning_ref.sort, or (words given) the same sort of the pairs the reach words keep"""
    if words is None:
        return R.sort(uv, depth, radius, W, H)
    gx, gy = R.grid(W, H)
    area, goff, gid, tile = R._pairs(uv, radius, W, H)
    x0, y0, x1, y1 = R.rect(uv, radius, W, H)
    w, h = np.maximum(x1 - x0, 1), np.maximum(y1 - y0, 1)
    wd = words.astype(np.int64)
    big = (wd >> 31) & 1
    assert np.array_equal(big == 1, area >= 32), "REACH_BIG marks exactly the rectangles of 32 tiles and more"
    sh, ncx, ncy = _cells(w, h)
    nbits = np.where(big == 1, ncx * ncy, area)
    assert ((wd & (REACH_BIG - 1)) >> nbits == 0).all(), "no flag past the rectangle's tiles / cells"
    k = np.arange(gid.size, dtype=np.int64) - np.repeat(goff - area, area)
    tx, ty = k % w[gid], k // w[gid]
    bit = np.where(big[gid] == 1, (ty >> sh[gid]) * ncx[gid] + (tx >> sh[gid]), k)
    keep = ((wd[gid] >> bit) & 1) == 1
    gid, tile = gid[keep], tile[keep]
    gcount = np.bincount(gid, minlength=radius.size).astype(np.int64)
    key = (tile.astype(np.uint64) << np.uint64(32)) | R.depth_bits(depth)[gid].astype(np.uint64)
    order = np.argsort(key, kind="stable")
    counts = np.bincount(tile, minlength=gx * gy).astype(np.int64)
    end = np.cumsum(counts)
    tr = np.stack([end - counts, end], axis=1)
    tr[counts == 0] = 0
    return R.Sorted(gid[order].astype(np.int32), tr.astype(np.int32), int(tile.size), gcount.astype(np.int32),
                    np.cumsum(gcount).astype(np.int32), order.astype(np.int32), tile[order])


# ================================================================== the library
def _run(frames, opacity, W, H, reach):
    """count + sort of a frame batch through the C ABI (pair-map mode) -> per-frame dicts"""
    lib, st = L.lib(), L.stream()
    F, P = len(frames), frames[0][2].size
    gx, gy = R.grid(W, H)
    T = gx * gy
    uv, depth, radius, conic = (_t(np.stack([fr[k] for fr in frames])) for k in range(4))
    op = _t(opacity)
    scratch = torch.empty(F * lib.splat_bin_scratch_bytes(P, W, H), dtype=torch.uint8, device="cuda")
    tr, m, gcount, words = _full(F * T * 2).view(F, T, 2), _full(F), _full(F * P), _full(F * P)
    if reach:
        L.check(lib.splat_bin_count_batch_reach(F, P, L.ptr(uv), L.ptr(radius), L.ptr(conic), L.ptr(op), 0,
                                                W, H, L.ptr(scratch), L.ptr(tr), L.ptr(m), L.ptr(gcount), L.ptr(words), st))
    else:
        L.check(lib.splat_bin_count_batch(F, P, L.ptr(uv), L.ptr(radius), W, H, L.ptr(scratch), L.ptr(tr), L.ptr(m), st))
    Ms = _n(m).tolist()
    cap = max(max(Ms), 0) + 64
    keys, idx, owner, slot = _full(F * cap, torch.int64), _full(F * cap), _full(F * cap), _full(F * cap)
    goff, ovf = _full(F * P), torch.zeros(1, dtype=torch.int32, device="cuda")
    if reach:
        L.check(lib.splat_bin_sort_batch_reach(F, P, L.ptr(uv), L.ptr(depth), L.ptr(radius), L.ptr(words), W, H,
                                               L.ptr(scratch), L.ptr(tr), cap, L.ptr(keys), L.ptr(idx), L.ptr(ovf),
                                               L.ptr(goff), L.ptr(owner), L.ptr(slot), st))
    else:
        L.check(lib.splat_bin_sort_batch(F, P, L.ptr(uv), L.ptr(depth), L.ptr(radius), W, H, L.ptr(scratch),
                                         L.ptr(tr), cap, L.ptr(keys), L.ptr(idx), L.ptr(ovf), L.ptr(goff), L.ptr(owner),
                                         L.ptr(slot), st))
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    tr, idx, slot, owner = _n(tr), _n(idx).reshape(F, cap), _n(slot).reshape(F, cap), _n(owner).reshape(F, cap)
    goff, gcount, words = _n(goff).reshape(F, P), _n(gcount).reshape(F, P), _n(words).reshape(F, P).view(np.uint32)
    return [dict(M=Ms[f], tr=tr[f], idx=idx[f], slot=slot[f], owner=owner[f], goff=goff[f], gcount=gcount[f], words=words[f])
            for f in range(F)]


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("slot_keys", [0, 1], ids=["packed", "slot_keys"])
@pytest.mark.parametrize("reach", [False, True], ids=["full", "reach"])
@pytest.mark.parametrize("name", list(CASES))
def test_area_order_keeps_every_output(gpu, lib_option, name, reach, slot_keys, F):
    W, H, _ = CASES[name]
    frames, opacity = _frames(name, F)
    P = frames[0][2].size
    lib_option("bin_slot_keys", slot_keys)
    runs = []
    for short in (0, 1, 0, 1):
        lib_option("bin_short_segments", short)
        runs.append(_run(frames, opacity, W, H, reach))
    packed = (not slot_keys) and R.plan(P, W, H, F)["packed"]
    for f, (uv, depth, radius, conic) in enumerate(frames):
        what = f"{name}, frame {f} of {F}"
        got = runs[0][f]
        for other in runs[1:]:                                   # both segment lengths, each twice: equal in everything
            for k, v in got.items():
                assert np.array_equal(v, other[f][k]), (what, k)
        if reach:
            exp, known = _expected_words(uv, radius, conic, opacity, W, H)
            assert known.sum() * 4 > P or P < 8, what             # (a third of the opacities is 0.003 in every frame)
            assert np.array_equal(got["words"][known], exp[known]), what
            ref = _reference(uv, depth, radius, W, H, got["words"])
            assert np.array_equal(got["gcount"], ref.gcount), what
        else:
            ref = _reference(uv, depth, radius, W, H)
        M = ref.M
        assert got["M"] == M, what
        assert np.array_equal(got["tr"], ref.tile_range), what
        assert np.array_equal(got["goff"], ref.goff_incl), what
        assert np.array_equal(got["idx"][:M], ref.idx_sorted), what
        assert np.array_equal(got["slot"][:M], ref.slot_sorted), what
        assert (got["idx"][M:] == SENT).all() and (got["slot"][M:] == SENT).all(), what
        owner = np.full(got["owner"].size, SENT, np.int32)
        if not packed:                                           # slot keys: owner[slot] = Gaussian; packed keys leave it alone
            owner[:M] = np.repeat(np.arange(P, dtype=np.int32), ref.gcount)
        assert np.array_equal(got["owner"], owner), what


def test_the_cases_hold_what_they_are_there_for():
    """CPU-side facts of the case list (no library call)"""
    for name in ("one_class_waves", "one_class_waves_stored", "every_class", "every_class_2049"):
        W, H, build = CASES[name]
        uv, depth, radius = build()
        x0, y0, x1, y1 = R.rect(uv, radius, W, H)
        area = (x1 - x0) * (y1 - y0)
        assert (radius <= 0).any() and ((radius > 0) & (area == 0)).any() and (area >= 32).any() and (area == 1).any(), name
        if name.startswith("every_class"):
            for c, lo in enumerate(CLASS_LOWER):
                hi = CLASS_LOWER[c - 1] if c else 1 << 30
                assert ((area >= lo) & (area < hi)).any(), (name, lo)
        else:
            assert int((area >= 32).sum()) == 20 and int((area == 1).sum()) == 200
    assert CASES["every_class"][2]()[2].size == 512 and CASES["every_class_2049"][2]()[2].size == 2049
    assert R.plan(1300, W0, H0, 5)["chunk"] == 1300 and R.plan(1300, W0, H0, 1)["chunk"] == 434
    assert R.plan(2049, W0, H0, 5)["chunk"] == 1025 and not R.plan(5, WG, HG)["lds"]
