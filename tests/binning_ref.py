"""Independent reference of tile binning + per-tile depth sort (csrc/binning.hip), numpy only and vectorised.

The operation (reference: dptr/gs/sort_gaussian.py:42-52, src/sort_gaussian.cu:16-70, include/utils.h:17-37): every Gaussian
with radius > 0 makes one (Gaussian, tile) pair per tile of its rectangle, in row-major order of the rectangle; the pairs are
sorted by the 64-bit key (tile << 32 | depth bits); a tile's slice of the sorted list is its range, tiles without pairs keep
(0, 0).  The library's order is that of a STABLE sort (equal tile and depth bits: ascending Gaussian id).

Nothing here loops over Gaussians: the pairs are laid out Gaussian-major with ``np.repeat`` on the rectangle areas, so that the
Gaussian-major position of a pair IS its slot (goff_excl[id] + k, k-th tile of the rectangle), and one stable argsort of the
keys gives idx_sorted and slot_sorted together.  Every expected value is an integer: every comparison is exact.

INPUT DOMAIN (every case below stays inside it):
  * depth: sign bit clear (+0, denormals, +inf included), no NaN.  The reference sign-extends the depth word into the key
    (src/sort_gaussian.cu:33) and negative depths never pass the near cull, so the order of negative words is nobody's contract;
  * uv: finite, and |uv| + |radius| + 16 below 2^24, so that every float -> int conversion is in range;
  * radius: any int32 of that size; radius <= 0 makes no pair.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

TILE = 16

# ---- the constants of csrc/binning.hip the case list is built around (test_binning_ref_cpu.py parses the source and asserts them)
BIN_BLOCK = 256
BIN_MAX_NB = 512
BIN_CHUNK = 512
BIN_CHUNK_BATCH = 2048
BIN_BATCH_FRAMES = 4
BIN_LDS_TILES = 12288
BIN_GLOBAL_BLOCKS = 2048
SORT_BLOCK = 256
COLSCAN_COLS = 32
COLSCAN_GROUPS = 1024 // COLSCAN_COLS
TILESCAN_THREADS = 1024


def grid(W: int, H: int):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def rect(uv, radius, W: int, H: int):
    """tile rectangle [x0, x1) x [y0, y1) of every Gaussian (get_rect, include/utils.h:17-37; tile_rect, csrc/common.h): float32
    arithmetic in the reference's operation order, truncation toward zero, clamp to [0, gx] / [0, gy]; radius <= 0: no tiles"""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    r = np.asarray(radius, np.int32).reshape(-1)
    gx, gy = grid(W, H)
    fr, t16, one = r.astype(np.float32), np.float32(TILE), np.float32(1.0)
    px, py = uv[:, 0], uv[:, 1]

    def lo(p, g):
        return np.clip(np.trunc((p - fr) / t16).astype(np.int64), 0, g)

    def hi(p, g):
        return np.clip(np.trunc((((p + fr) + t16) - one) / t16).astype(np.int64), 0, g)

    x0, y0, x1, y1 = lo(px, gx), lo(py, gy), hi(px, gx), hi(py, gy)
    dead = r <= 0
    for a in (x0, y0, x1, y1):
        a[dead] = 0
    return x0, y0, x1, y1


def depth_bits(depth):
    d = np.ascontiguousarray(np.asarray(depth, np.float32).reshape(-1))
    bits = d.view(np.uint32)
    assert not np.isnan(d).any() and not (bits >> 31).any(), "outside the input domain: NaN or a set sign bit"
    return bits


def _pairs(uv, radius, W, H):
    """Gaussian-major pairs: (gcount, goff_incl, id of every pair, tile of every pair)"""
    gx, _ = grid(W, H)
    x0, y0, x1, y1 = rect(uv, radius, W, H)
    w, h = x1 - x0, y1 - y0
    area = np.maximum(w, 0) * np.maximum(h, 0)
    goff_incl = np.cumsum(area)
    M = int(goff_incl[-1]) if area.size else 0
    gid = np.repeat(np.arange(area.size, dtype=np.int64), area)
    k = np.arange(M, dtype=np.int64) - np.repeat(goff_incl - area, area)
    wr = np.repeat(w, area)
    tile = (np.repeat(y0, area) + k // np.maximum(wr, 1)) * gx + np.repeat(x0, area) + k % np.maximum(wr, 1)
    return area, goff_incl, gid, tile


class Sorted(NamedTuple):
    idx_sorted: np.ndarray    # [M] int32
    tile_range: np.ndarray    # [T, 2] int32, empty tiles (0, 0)
    M: int
    gcount: np.ndarray        # [P] int32 tiles per Gaussian
    goff_incl: np.ndarray     # [P] int32 = cumsum(gcount)
    slot_sorted: np.ndarray   # [M] int32: goff_excl[id] + k of every sorted entry
    tile_sorted: np.ndarray   # [M] int64: tile of every sorted entry


def sort(uv, depth, radius, W: int, H: int) -> Sorted:
    gx, gy = grid(W, H)
    T = gx * gy
    area, goff_incl, gid, tile = _pairs(uv, radius, W, H)
    key = (tile.astype(np.uint64) << np.uint64(32)) | depth_bits(depth)[gid].astype(np.uint64)
    order = np.argsort(key, kind="stable")      # pairs are Gaussian-major: stable = ascending id among equal keys
    counts = np.bincount(tile, minlength=T).astype(np.int64)
    end = np.cumsum(counts)
    tr = np.stack([end - counts, end], axis=1)
    tr[counts == 0] = 0
    return Sorted(gid[order].astype(np.int32), tr.astype(np.int32), int(tile.size), area.astype(np.int32),
                  goff_incl.astype(np.int32), order.astype(np.int32), tile[order])


def keys(uv, depth, radius, W: int, H: int):
    """(key [M] int64 = tile << 32 | depth bits, gaussian id [M] int32) of the reference-flow helper compute_gaussian_key:
    Gaussian-major, row-major inside the rectangle (src/sort_gaussian.cu:24-44)"""
    _, _, gid, tile = _pairs(uv, radius, W, H)
    key = (tile.astype(np.uint64) << np.uint64(32)) | depth_bits(depth)[gid].astype(np.uint64)
    return key.view(np.int64), gid.astype(np.int32)


# ================================================================== inputs
_DENORMAL = np.float32(1e-42)
SPECIAL_DEPTHS = np.array([0.0, _DENORMAL, 0.5, np.nextafter(np.float32(0.5), np.float32(1.0)), 1.0, 3e38, np.inf], np.float32)
assert 0 < _DENORMAL < np.finfo(np.float32).tiny


def random_inputs(P: int, W: int, H: int, rmax: int, seed: int):
    """centres over the image and a margin around it, radii in [-2, rmax] (about one in twelve <= 0), depths: two thirds
    uniform, the rest from a handful of values (ties) and the special words"""
    rng = np.random.default_rng(seed)
    m = 2.0 * rmax + 8.0
    uv = np.stack([rng.uniform(-m, W + m, P), rng.uniform(-m, H + m, P)], axis=1).astype(np.float32)
    radius = rng.integers(-2, rmax + 1, P).astype(np.int32)
    radius[rng.random(P) < 0.04] = 0
    depth = rng.uniform(0.01, 30.0, P).astype(np.float32)
    pick = rng.random(P)
    few = rng.uniform(0.5, 2.0, 5).astype(np.float32)
    depth = np.where(pick < 0.2, few[rng.integers(0, 5, P)], depth)
    depth = np.where(pick > 0.9, SPECIAL_DEPTHS[rng.integers(0, SPECIAL_DEPTHS.size, P)], depth).astype(np.float32)
    return uv, depth, radius


class Case(NamedTuple):
    name: str
    branch: str     # the plan branch the case is there for
    W: int
    H: int
    P: int
    rmax: int       # largest radius (small at large P: M stays below about a million)

    @property
    def T(self):
        gx, gy = grid(self.W, self.H)
        return gx * gy


def _c(name, branch, gx, gy, P, rmax, dw=0, dh=0, H=None):
    return Case(name, branch, TILE * gx - dw, (TILE * gy - dh) if H is None else H, P, rmax)


# (grid, P) cases of the plan branches.  Thin images (one or two tile rows) make the large grids cheap.
PLAN_CASES = [
    # ---- LDS path (T <= BIN_LDS_TILES): rows of the count matrix NB = min(ceil(P / BIN_CHUNK), BIN_MAX_NB)
    _c("T1_P1", "one tile, one Gaussian: NB = 1, every scan of length one", 1, 1, 1, 40),
    _c("T1_P255", "one tile: one short of a BIN_BLOCK in the single chunk", 1, 1, 255, 40, dw=3, dh=7),
    _c("T1023_P256", "T one short of the tile scan's 1024 threads; a chunk of exactly BIN_BLOCK", 33, 31, 256, 60),
    _c("T1024_P257", "T = the tile scan's 1024 threads (carry after a full trip, no second); second scatter trip of one", 32, 32, 257, 60),
    _c("T1025_P512", "tile scan's second trip (T > 1024); P = BIN_CHUNK: still one row", 41, 25, 512, 60),
    _c("T819odd_P513", "W and H no multiples of 16; P = BIN_CHUNK + 1: two rows, chunk 257", 63, 13, 513, 40, dw=5, dh=9),
    _c("T1025_P16385", "NB = 33 > COLSCAN_GROUPS: column scan with two rows per group", 41, 25, 16385, 12),
    _c("T12288x1_P1", "last LDS size (48 KiB of counters + static LDS) as 12288 x 1, H = 7", 12288, 1, 1, 300, H=7),
    _c("T12288x1_P16385", "last LDS size; NB = 33", 12288, 1, 16385, 30, H=7),
    _c("T6144x2_P257", "last LDS size as 6144 x 2", 6144, 2, 257, 200),
    _c("T6144x2_P262144", "last LDS size; P = BIN_MAX_NB * BIN_CHUNK: 512 rows of 512, 16 rows per column-scan group", 6144, 2, 262144, 6),
    _c("T1024_P262145", "BIN_MAX_NB cap: chunk 513 (third scatter trip of one); packed keys (19 + 10 bits)", 32, 32, 262145, 6),
    _c("T12288x1_P262145", "BIN_MAX_NB cap on the last LDS size; bits(P) + bits(T) = 33: natural fall-back to slot keys", 12288, 1, 262145, 6, H=7),
    # ---- global-atomic path (T > BIN_LDS_TILES): nchunk = min(ceil(P / BIN_BLOCK), BIN_GLOBAL_BLOCKS)
    _c("T12289x1_P1", "first global size: one workgroup, one Gaussian", 12289, 1, 1, 300),
    _c("T12289x1_P257", "first global size: nchunk = 2, chunk 129", 12289, 1, 257, 200),
    _c("T97x127_P257", "global path in two dimensions (ty * gx + tx)", 97, 127, 257, 120),
    _c("T97x127_P5000", "global path in two dimensions, nchunk = 20", 97, 127, 5000, 60, dw=9, dh=3),
    _c("T12289x1_P262145", "global path: nchunk = 1025, the tile scan's chunk loop takes its second trip", 12289, 1, 262145, 6),
    _c("T97x127_P524800", "global path: nchunk capped at BIN_GLOBAL_BLOCKS = 2048, chunk 257 > BIN_BLOCK", 97, 127, 524800, 4),
]
PLAN_BY_NAME = {c.name: c for c in PLAN_CASES}


def plan(P: int, W: int, H: int, F: int = 1):
    """the branch facts of make_plan (csrc/binning.hip), restated from the constants above: what a case's name promises"""
    gx, gy = grid(W, H)
    T = gx * gy
    lds = T <= BIN_LDS_TILES
    nb = min(max(-(-P // BIN_CHUNK), 1), BIN_MAX_NB) if lds else 1
    if lds and F >= BIN_BATCH_FRAMES:
        nb = min(nb, max(-(-P // BIN_CHUNK_BATCH), 1))
    nchunk = nb if lds else max(1, min(-(-P // BIN_BLOCK), BIN_GLOBAL_BLOCKS))
    chunk = max(-(-P // nchunk), 1)
    bits = lambda n: max(1, int(n - 1).bit_length())
    return dict(T=T, lds=lds, NB=nb, nchunk=nchunk, chunk=chunk, rpg=-(-nb // COLSCAN_GROUPS),
                packed=bits(P) + bits(T) <= 32)


def case_inputs(case: Case):
    """(uv, depth, radius) of a plan case: seeded by its name, with one Gaussian covering every tile in the larger ones"""
    seed = int.from_bytes(case.name.encode(), "little") % (1 << 31)
    uv, depth, radius = random_inputs(case.P, case.W, case.H, case.rmax, seed)
    if 256 <= case.P <= 20000:      # one splat over the whole grid (area = T)
        uv[case.P // 2] = (case.W / 2, case.H / 2)
        radius[case.P // 2] = max(case.W, case.H)
    if case.P == 1:
        uv[0] = (case.W / 3, case.H / 2)
        radius[0] = case.rmax
    return uv, depth, radius


@functools.lru_cache(maxsize=None)
def case_reference(name: str) -> Sorted:
    c = PLAN_BY_NAME[name]
    uv, depth, radius = case_inputs(c)
    return sort(uv, depth, radius, c.W, c.H)


# ---- (b) every list length on purpose: one tile per length on a thin image
LIST_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025,
                1535, 1536, 1537, 2047, 2048, 2049, 2050, 4095, 4096, 4097, 5600, 6143, 6144, 6145, 8191, 8192, 8193, 16385, 20000]
DEPTH_PATTERNS = ["ascending", "descending", "equal", "five_values", "special"]


def length_inputs(pattern: str, seed: int = 5):
    """-> (uv, depth, radius, W, H, tile_of_gaussian): tile t holds LIST_LENGTHS[t] Gaussians of radius 1 at its centre; ids are
    interleaved across the tiles by a seeded permutation"""
    rng = np.random.default_rng(seed)
    n = np.asarray(LIST_LENGTHS)
    P = int(n.sum())
    tile = np.repeat(np.arange(n.size), n)[rng.permutation(P)]
    uv = np.stack([TILE * tile + 8.0, np.full(P, 8.0)], axis=1).astype(np.float32)
    radius = np.ones(P, np.int32)
    if pattern == "ascending":
        depth = np.linspace(0.1, 50.0, P, dtype=np.float32)
        assert (np.diff(depth) > 0).all()
    elif pattern == "descending":
        depth = np.linspace(50.0, 0.1, P, dtype=np.float32)
        assert (np.diff(depth) < 0).all()
    elif pattern == "equal":
        depth = np.full(P, 1.25, np.float32)
    elif pattern == "five_values":
        depth = np.array([0.5, 0.75, 1.0, 2.5, 7.0], np.float32)[rng.integers(0, 5, P)]
    elif pattern == "special":
        depth = SPECIAL_DEPTHS[rng.integers(0, SPECIAL_DEPTHS.size, P)]
    else:
        raise ValueError(pattern)
    return uv, depth, radius, TILE * n.size, TILE, tile


@functools.lru_cache(maxsize=None)
def length_reference(pattern: str) -> Sorted:
    uv, depth, radius, W, H, _ = length_inputs(pattern)
    return sort(uv, depth, radius, W, H)


# ---- (c) rectangle edges
def edge_inputs(W: int, H: int, seed: int = 11):
    """Gaussians on the edges of the rectangle rule, for a grid of at least 3 x 1 tiles"""
    rng = np.random.default_rng(seed)
    f = np.float32
    up = lambda x: np.nextafter(f(x), f(np.inf))
    dn = lambda x: np.nextafter(f(x), f(-np.inf))
    gx, gy = grid(W, H)
    rows = []       # (px, py, r)
    bx = [0.0, 16.0, 32.0, float(TILE * (gx - 1)), float(TILE * gx), float(W)]
    by = [0.0, 16.0, float(TILE * (gy - 1)), float(TILE * gy), float(H)]
    for x in bx:                       # centres exactly on tile borders and one ulp either side
        for y in by:
            for r in (1, 3, 16, 17):
                for px in (dn(x), f(x), up(x)):
                    for py in (dn(y), f(y), up(y)):
                        rows.append((px, py, r))
    for r in (1, 5, 16, 21):           # uv - r and uv + r exact multiples of 16, and one ulp either side of that
        for k in (0, 1, 2, gx - 1, gx):
            for x in (TILE * k + r, TILE * k - r):
                for px in (dn(x), f(x), up(x)):
                    rows.append((px, f(TILE * min(k, gy) + r), r))
                    rows.append((f(5.0), px, r))
    for px, r in ((-3.0, 5), (-3.0, 10), (-0.5, 15), (-15.0, 16), (-14.0, 1), (-1.0, 1), (-8.0, 20)):   # (px - r) / 16 in (-1, 0):
        rows.append((f(px), f(4.0), r))                                                                    # truncation, not floor
        rows.append((f(4.0), f(px), r))
        rows.append((f(px), f(px), r))
    for px, py, r in ((-100.0, 5.0, 5), (W + 200.0, 5.0, 7), (5.0, -60.0, 9), (5.0, H + 90.0, 30), (-17.0, -17.0, 1),
                      (W + 16.0, H + 16.0, 2)):             # r > 0, the rectangle empty
        rows.append((f(px), f(py), r))
    for r in (0, -1, -7, -(1 << 20)):  # no tiles whatever the centre
        rows.append((f(W / 2), f(H / 2), r))
        rows.append((f(-3.0), f(2.0), r))
    big = max(W, H) + 16               # the whole grid (area = T), three times: ties over every tile
    rows += [(f(W / 2), f(H / 2), big), (f(0.0), f(0.0), 2 * big), (f(W), f(H), 2 * big)]
    for _ in range(300):               # radius 1 anywhere
        rows.append((f(rng.uniform(-2, W + 2)), f(rng.uniform(-2, H + 2)), 1))
    a = np.array(rows, np.float64)
    uv = a[:, :2].astype(np.float32)
    radius = a[:, 2].astype(np.int32)
    depth = SPECIAL_DEPTHS[rng.integers(0, SPECIAL_DEPTHS.size, radius.size)]
    depth[::3] = rng.uniform(0.1, 9.0, depth[::3].size).astype(np.float32)
    return uv, depth, radius


# ---- (f), (g) one scene on both sides of the BIN_LDS_TILES boundary: a 6144 x 2 grid (LDS path) and a 6145 x 2 grid (global path)
REACH_GX = BIN_LDS_TILES // 2


def reach_inputs(seed: int = 23):
    """-> (uv, depth, radius, conic, opacity) with every rectangle left of tile column REACH_GX on an image of two tile rows:
    about 40 rectangles of at least 32 tiles (the cell form of the reach word), elongated splats, a block with opacity 0.0035"""
    rng = np.random.default_rng(seed)
    n_big, n_long, n_small = 44, 400, 2600
    P = n_big + n_long + n_small
    s1 = np.concatenate([rng.uniform(90.0, 160.0, n_big), rng.uniform(8.0, 30.0, n_long), rng.uniform(0.4, 9.0, n_small)])
    s2 = np.concatenate([s1[:n_big] * rng.choice([1.0, 0.08], n_big), s1[n_big:n_big + n_long] * 0.1, s1[n_big + n_long:] * rng.uniform(0.5, 1.0, n_small)])
    th = rng.uniform(0.0, np.pi, P)
    c, s = np.cos(th), np.sin(th)
    a = c * c * s1 ** 2 + s * s * s2 ** 2
    b = c * s * (s1 ** 2 - s2 ** 2)
    d = s * s * s1 ** 2 + c * c * s2 ** 2
    det = a * d - b * b
    conic = np.stack([d / det, -b / det, a / det], axis=1).astype(np.float32)
    radius = np.ceil(3.0 * np.maximum(s1, s2)).astype(np.int32)
    W = TILE * REACH_GX
    x = np.where(rng.random(P) < 0.5, rng.uniform(2000.0, 6000.0, P), rng.uniform(600.0, W - 600.0, P))
    uv = np.stack([x, rng.uniform(-4.0, 36.0, P)], axis=1).astype(np.float32)
    assert (uv[:, 0] + radius + TILE < W).all() and int(radius.max()) < 500
    opacity = rng.uniform(0.05, 1.0, P).astype(np.float32)
    opacity[n_big + n_long:n_big + n_long + 300] = 0.0035        # below 1/255: no pair at all
    depth = rng.uniform(0.1, 20.0, P).astype(np.float32)
    depth[::7] = 1.5
    order = rng.permutation(P)
    return uv[order], depth[order], radius[order], conic[order], opacity[order]
