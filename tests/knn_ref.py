"""float64 brute-force K nearest neighbours and the rules a float32 search is accepted by: the reference the grid search
(knn.knn_points / distCUDA2) and the brute-force batch search (knn.knn_brute_batch / arap.pair_connectivity) are checked
against.  Pure numpy, no GPU; nothing here is shared with the kernels or with the C oracle.

``check`` states what "the K nearest neighbours in float32" means without a share of mismatches that are let through.  With
u = 2^-24 and D(i) the float64 squared distance of point i from the row's query:
  1. a row holds min(K, M) distinct valid ids, then -1 / 0.0 padding; its distances ascend;
  2. |dists[r] - D(idx[r])| <= 6 u D(idx[r]): the kernels round a difference and a square per axis (3 u per term: the
     difference enters the square twice) and two additions of non-negative terms (2 u), which is 5 u to first order; 6 u carries
     the second-order terms.  FMA contraction only removes roundings.  There is no absolute term: the inputs keep their non-zero
     squared distances far above float32's subnormals;
  3. the row is a nearest set: D(idx[K-1]) <= D64_K (1 + 12 u), and no point outside the row has D < D(idx[K-1]) (1 - 12 u)
     -- twice the bound of rule 2, because both sides of the kernel's comparison may be off;
  4. idx[r] < idx[r+1] wherever dists[r] == dists[r+1] bit for bit (the kernels' own tie rule);
  5. ``exact=True`` (inputs whose squared distances are exact in float32): idx and dists equal knn64's exactly.

Measured on an MI355X (worst |dists - D| / (u D) over every case of tests/test_gpu_knn_reference.py): grid search 4.21 u,
brute-force batch search 4.10 u (the compiler contracts some products into FMAs, which shifts single errors but stays under the
first-order 5 u); the float32 numpy model below (no FMA) 3.36 u; distCUDA2 3.40 u of its 8 u.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

U = 2.0 ** -24          # float32 unit roundoff
_THREADS = max(1, min(8, os.cpu_count() or 1))


def _dist64(q: np.ndarray, p: np.ndarray) -> np.ndarray:
    """[rows, M] float64 squared distances (q, p float64)"""
    d = np.square(q[:, 0:1] - p[None, :, 0])
    d += np.square(q[:, 1:2] - p[None, :, 1])
    d += np.square(q[:, 2:3] - p[None, :, 2])
    return d


def _rows_per_chunk(M: int) -> int:
    return max(1, 2_000_000 // max(M, 1))       # 16 MB of float64 per chunk: 512 x 300 000 never exists at once


def knn64(query, points, K: int):
    """(dists [N, K] float64, idx [N, K] int64): the K nearest of ``points`` [M, 3] for every row of ``query`` [N, 3], squared
    distances in float64 from the float32 inputs, ordered by (distance, index); columns past M are 0 / -1"""
    q = np.asarray(query, np.float32).astype(np.float64).reshape(-1, 3)
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    N, M = q.shape[0], p.shape[0]
    nv = min(K, M)
    dists = np.zeros((N, K), np.float64)
    idx = np.full((N, K), -1, np.int64)
    if nv == 0 or N == 0:
        return dists, idx
    step = _rows_per_chunk(M)

    def work(a: int) -> None:
        d = _dist64(q[a:a + step], p)
        kth = np.partition(d, nv - 1, axis=1)[:, nv - 1]
        for r in range(d.shape[0]):
            cand = np.flatnonzero(d[r] <= kth[r])               # ascending ids: a stable sort keeps ties by index
            o = cand[np.argsort(d[r, cand], kind="stable")[:nv]]
            idx[a + r, :nv] = o
            dists[a + r, :nv] = d[r, o]

    starts = range(0, N, step)
    if _THREADS > 1 and len(starts) > 1:
        with ThreadPoolExecutor(_THREADS) as ex:
            list(ex.map(work, starts))
    else:
        for a in starts:
            work(a)
    return dists, idx


def check(dists, idx, query, points, K: int, exact: bool = False, ref=None, what: str = "") -> float:
    """raise AssertionError (naming the first offending row) unless ``dists`` / ``idx`` [N, K] are the K nearest of ``points`` for
    every row of ``query`` by the rules of the module docstring.  ``ref``: knn64(query, points, K' >= K) if already at hand.
    Returns the worst distance error in units of u D."""
    q = np.asarray(query, np.float32).astype(np.float64).reshape(-1, 3)
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    got_d = np.asarray(dists)
    got_i = np.asarray(idx).astype(np.int64)
    N, M = q.shape[0], p.shape[0]
    nv = min(K, M)
    assert got_d.shape == (N, K) and got_i.shape == (N, K), (what, got_d.shape, got_i.shape, (N, K))
    assert got_d.dtype == np.float32, (what, got_d.dtype)
    d64, i64 = ref if ref is not None else knn64(query, points, K)
    d64, i64 = d64[:, :K], i64[:, :K]
    assert d64.shape == (N, K)

    def fail(rule: str, bad: np.ndarray) -> None:
        r = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what} rule {rule}: {int(bad.sum())} of {N} rows; first row {r}: idx {got_i[r].tolist()} dists "
                             f"{got_d[r].tolist()}; float64 idx {i64[r].tolist()} dists {d64[r].tolist()}")

    # 1. valid distinct ids, padding, ascending
    v, pad = got_i[:, :nv], got_i[:, nv:]
    bad = ((v < 0) | (v >= M)).any(axis=1) | (pad != -1).any(axis=1) | (got_d[:, nv:] != 0).any(axis=1)
    sv = np.sort(v, axis=1)
    bad |= (sv[:, 1:] == sv[:, :-1]).any(axis=1)
    bad |= ~(np.diff(got_d[:, :nv].astype(np.float64), axis=1) >= 0).all(axis=1)          # (a NaN fails too)
    if bad.any():
        fail("1 (distinct valid ids, padding, ascending)", bad)
    if nv == 0:
        return 0.0
    # 2. the distances
    D = np.square(q[:, None, :] - p[v]).sum(-1)                                              # [N, nv] float64
    err = np.abs(got_d[:, :nv].astype(np.float64) - D)
    bad = ~(err <= 6 * U * D).all(axis=1)
    if bad.any():
        fail("2 (|dists - D| <= 6 u D)", bad)
    worst = float(np.max(np.divide(err, U * D, out=np.zeros_like(err), where=D > 0)))
    # 3. a nearest set
    last = D[:, nv - 1]
    bad = ~(last <= d64[:, nv - 1] * (1 + 12 * U))
    if bad.any():
        fail("3 (D(idx[K-1]) <= D64_K (1 + 12 u))", bad)
    # the nearest point outside the row is the first float64 neighbour the row lacks: if it lacks none the row is the
    # float64 set, and every other point is at D64_K or further
    inrow = (i64[:, :nv, None] == v[:, None, :]).any(axis=2)
    first_out = np.where(inrow, np.inf, d64[:, :nv]).min(axis=1)
    bad = first_out < last * (1 - 12 * U)
    if bad.any():
        fail("3 (a point outside the row is nearer than D(idx[K-1]) (1 - 12 u))", bad)
    # 4. ties in the row's own distances -> smaller index first
    tie = got_d[:, 1:nv] == got_d[:, :nv - 1]
    bad = (tie & ~(v[:, 1:] > v[:, :-1])).any(axis=1)
    if bad.any():
        fail("4 (equal distances -> smaller index first)", bad)
    # 5. exact inputs
    if exact:
        bad = (got_i != i64).any(axis=1) | (got_d.astype(np.float64) != d64).any(axis=1)
        if bad.any():
            fail("5 (exact inputs: idx and dists equal the float64 search)", bad)
    return worst


def connectivity64(points, sample, K: int = 5, radius: float = 0.1, least_edge_num: int = 3):
    """rows ``sample`` of the neighbour table of ``cal_connectivity_from_points(points, radius, K, least_edge_num)``: the K + 1
    nearest by knn64, the first column (the vertex itself) dropped, columns >= least_edge_num cut (-1) where d >= radius^2.
    Returns (nbr [S, K] int64, d [S, K] float64 = the distances before the cut)"""
    pts = np.asarray(points, np.float32)
    d, i = knn64(pts[np.asarray(sample)], pts, K + 1)
    d, i = d[:, 1:], i[:, 1:].copy()
    cut = d >= float(radius) ** 2
    cut[:, :least_edge_num] = False
    i[cut] = -1
    return i, d


def model32(query, points, K: int):
    """numpy float32 model of the kernels' arithmetic, brute force: (qx - px)^2 + (qy - py)^2 + (qz - pz)^2 with every operation
    rounded to float32 (no FMA), ordered by (distance, index), 0 / -1 padding -> (dists float32, idx int64)"""
    q = np.asarray(query, np.float32).reshape(-1, 3)
    p = np.asarray(points, np.float32).reshape(-1, 3)
    N, M = q.shape[0], p.shape[0]
    nv = min(K, M)
    dists = np.zeros((N, K), np.float32)
    idx = np.full((N, K), -1, np.int64)
    step = _rows_per_chunk(M) * 2
    ids = np.arange(M)
    for a in range(0, N, step):
        qq = q[a:a + step]
        dx, dy, dz = qq[:, 0:1] - p[None, :, 0], qq[:, 1:2] - p[None, :, 1], qq[:, 2:3] - p[None, :, 2]
        d = dx * dx + dy * dy + dz * dz
        assert d.dtype == np.float32
        for r in range(d.shape[0]):
            o = np.lexsort((ids, d[r]))[:nv]
            idx[a + r, :nv] = o
            dists[a + r, :nv] = d[r, o]
    return dists, idx


# ------------------------------------------------------------------ input families (seeded; shared by the CPU and GPU tests)
def morton_order(uv: np.ndarray) -> np.ndarray:
    """stable argsort of the 2 x 15 bit Z-curve code of ``uv`` in [-1, 1]^2: the layout densify.spatial_order keeps the
    Gaussians in (index neighbours are mostly space neighbours)"""
    def spread(v):
        v = v.astype(np.uint32)
        v = (v | (v << 8)) & 0x00FF00FF
        v = (v | (v << 4)) & 0x0F0F0F0F
        v = (v | (v << 2)) & 0x33333333
        return (v | (v << 1)) & 0x55555555
    g = np.clip((np.asarray(uv, np.float64) + 1.0) * 16384.0, 0, 32767).astype(np.uint32)
    return np.argsort(spread(g[:, 0]) | (spread(g[:, 1]) << 1), kind="stable")


def lattice(seed: int = 0, integer: bool = False) -> np.ndarray:
    """the 16^3 grid / 16 in shuffled order plus 300 duplicated points (4396 points: two chunks, five tiles of the brute-force
    search): squared distances are multiples of 1/256, exact in float32, with ties at every rank and zero distances.
    ``integer``: the same lattice as integers shifted by -7 (exact too; points on the grid search's cell boundaries)"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))]
    g = np.concatenate([g, g[rng.integers(0, len(g), 300)]])
    g = g[rng.permutation(len(g))]
    return (g - 7).astype(np.float32) if integer else (g / 16.0).astype(np.float32)


def aniso_lattice(seed: int = 0) -> np.ndarray:
    """16 x 12 x 10 lattice with spacings 1/16, 2/16, 3/16, shuffled: squared distances are multiples of 1/256 (1: the two x
    neighbours; 4: +-2x and +-y; 5, 8, 9, ..), none near radius^2 = 0.01 = 2.56 / 256"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(16), 2 * np.arange(12), 3 * np.arange(10), indexing="ij"), -1).reshape(-1, 3)
    return (g[rng.permutation(len(g))] / 16.0).astype(np.float32)


def sheet(N: int, seed: int = 3, order: str = "morton", noise: float = 0.0, plane: bool = False) -> np.ndarray:
    """(u, v, 0.2 sin 3u cos 2v + 3), u, v uniform in [-1, 1]: the surface-like sets this project trains, in Morton order of
    (u, v) -- the training layout -- or in random order; ``noise``: normal offsets off the sheet; ``plane``: z = 3 exactly"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1, 1, size=(N, 2))
    z = np.full(N, 3.0) if plane else 0.2 * np.sin(3 * uv[:, 0]) * np.cos(2 * uv[:, 1]) + 3.0
    pts = np.stack([uv[:, 0], uv[:, 1], z], 1)
    if noise:
        pts = pts + noise * rng.normal(size=pts.shape)
    pts = pts.astype(np.float32)
    if order == "morton":
        return np.ascontiguousarray(pts[morton_order(uv)])
    assert order == "random"
    return pts


def clustered(N: int, seed: int = 3) -> np.ndarray:
    """twelve tight clusters and seven far outliers that stretch the grid"""
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(12, 3)) * 5
    c = (centers[rng.integers(0, 12, N)] + 0.01 * rng.normal(size=(N, 3))).astype(np.float32)
    c[:min(7, N)] = (rng.normal(size=(7, 3)) * 200)[:min(7, N)]
    return c


def offset(N: int, seed: int = 5) -> np.ndarray:
    """extent 1 around (1000, -2000, 500): float32 spacing 1.2e-4 there, the grid search's rounding slack is large"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-0.5, 0.5, size=(N, 3)) + np.array([1000.0, -2000.0, 500.0])).astype(np.float32)


def line(N: int) -> np.ndarray:
    p = np.zeros((N, 3), np.float32)
    p[:, 0] = np.linspace(0, 1, N)
    return p


def identical(N: int) -> np.ndarray:
    return np.tile(np.array([[0.3, -1.0, 2.0]], np.float32), (N, 1))


def cloud(N: int, seed: int = 7) -> np.ndarray:
    return np.random.default_rng(seed + N).normal(size=(N, 3)).astype(np.float32)


TINY = (1, 2, 5, 7, 9, 17, 127, 128, 129)


def families(N: int):
    """[(name, points, exact)]: every family at about N points (the lattices have their own size)"""
    out = [("lattice", lattice(), True), ("lattice_int", lattice(integer=True), True),
           ("sheet_morton", sheet(N), False), ("sheet_random", sheet(N, order="random"), False),
           ("clustered", clustered(N), False), ("offset", offset(N), False), ("line", line(min(N, 4000)), False),
           ("identical", identical(min(N, 5000)), True)]
    out += [(f"tiny{n}", cloud(n), False) for n in TINY]
    return out
