"""The neighbour searches against an independent float64 brute force (tests/knn_ref.py: knn64 + check, no share of mismatches
let through): knn.knn_brute_batch / arap.pair_connectivity at the shapes the training step calls them with (Morton-ordered sheets,
sorted queries drawn with replacement, a strided view, 74 chunks), around every constant of the kernels, on exact lattices
(ties across tiles, chunks and lanes) and degenerate sets; knn.knn_points / distCUDA2 on the same families."""
import numpy as np
import pytest
import torch

import knn_ref as R
from splatter_a_video_amd.arap import pair_connectivity
from splatter_a_video_amd.knn import distCUDA2, knn_brute_batch, knn_points

pytestmark = pytest.mark.gpu
WORST = {"brute": 0.0, "grid": 0.0}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _note(kind, w):
    WORST[kind] = max(WORST[kind], w)
    print(f"[{kind}] worst distance error so far {WORST[kind]:.2f} u")


def _brute(sets, q, K, strided=True):
    """knn_brute_batch of B equally sized sets; ``strided``: read in place from the first half of a [B, 2, N, 3] buffer, as the
    training step reads position(ids1) of its pairs"""
    pts = np.stack(sets)
    if strided:
        buf = _t(np.stack([pts, np.full_like(pts, 1e9)], 1))              # the other half must never be read as a candidate
        view = buf[:, 0]
        assert not view.is_contiguous() or pts.shape[0] == 1
    else:
        view = _t(pts)
    d, i = knn_brute_batch(view, _t(np.asarray(q, np.int64)), K)
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and d.shape == i.shape == (pts.shape[0], np.shape(q)[1], K)
    return d.cpu().numpy(), i.cpu().numpy()


def _check_brute(sets, q, K, exact=False, what="", ks=None, strided=True):
    """one reference at the largest K serves every smaller K (the order is by (distance, index))"""
    q = np.asarray(q, np.int64)
    ks = ks or [K]
    refs = [R.knn64(s[q[b]], s, max(ks)) for b, s in enumerate(sets)]
    for k in ks:
        d, i = _brute(sets, q, k, strided)
        for b, s in enumerate(sets):
            _note("brute", R.check(d[b], i[b], s[q[b]], s, k, exact=exact, ref=refs[b], what=f"{what} N={len(s)} K={k} b={b}"))
    return d, i


@pytest.mark.parametrize("N", [300_000, 262_145])
def test_brute_batch_at_the_training_steps_call(N):
    """N = 300 000 is 74 chunks, 262 145 is 65: the merge kernel's lanes take a second chunk"""
    rng = np.random.default_rng(N)
    B, S, K = 3, 512, 6
    sets = [R.sheet(N, seed=10 + b) for b in range(B)]
    q = rng.integers(0, N, size=(B, S))
    q[:, 100:120] = q[:, 200:220]                                         # drawn with replacement: duplicates (20 made sure of)
    q[:, 120:123] = q[:, 200:201]
    q = np.sort(q, axis=1)
    d, i = _check_brute(sets, q, K, what="morton sheet, sorted queries")
    # the same queries unsorted: every (query, point) distance is the same arithmetic, so the rows are the same bits
    perm = np.stack([rng.permutation(S) for _ in range(B)])
    d2, i2 = _brute(sets, np.take_along_axis(q, perm, 1), K)
    assert np.array_equal(d2, np.take_along_axis(d, perm[:, :, None], 1))
    assert np.array_equal(i2, np.take_along_axis(i, perm[:, :, None], 1))
    if N == 300_000:      # the points in random order (loose bounds, no tile skipped): the same neighbours under the relabelling
        order = [rng.permutation(N) for _ in range(B)]
        inv = [np.argsort(o) for o in order]
        d3, i3 = _check_brute([s[o] for s, o in zip(sets, order)], np.stack([inv[b][q[b]] for b in range(B)]), K,
                              what="random order")
        for b in range(B):
            notie = (np.diff(d[b], axis=1) > 0).all(axis=1)
            assert np.array_equal(d3[b], d[b]) and np.array_equal(order[b][i3[b]][notie], i[b][notie])


@pytest.mark.parametrize("N", [1, 5, 7, 8, 9, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 8200])
def test_brute_batch_around_the_kernels_constants(N):
    """window 128, tile 1024, chunk 4096, 8 points per scalar trip, 4 waves / 256 queries per block, K registers 8; fewer points
    than K (padding); sample = arange(N), the step's call when N <= S"""
    rng = np.random.default_rng(N)
    sets = [R.sheet(N, seed=20), R.sheet(N, seed=21)]
    ks = list(range(1, 9))
    for S in (1, 3, 4, 5, 255, 256, 257):
        q = np.sort(rng.integers(0, N, size=(2, S)), axis=1)
        _check_brute(sets, q, 8, ks=ks, what=f"S={S}")
    _check_brute(sets, np.tile(np.arange(N), (2, 1)), 8, ks=ks, what="sample=arange(N)")
    _check_brute(sets[:1], np.arange(N)[None, ::-1].copy(), 8, ks=[1, 6, 8], what="B=1 contiguous, descending", strided=False)
    c = R.cloud(N)
    _check_brute([c], rng.integers(0, N, size=(1, 300)), 8, ks=[2, 6], what="normal cloud, unsorted")


@pytest.mark.parametrize("integer", [False, True])
def test_brute_batch_exact_lattice_ties(integer):
    """4396 points = two chunks, five tiles: exact ties at every rank cross tile, chunk and lane boundaries"""
    lat = R.lattice(integer=integer)
    assert len(lat) == 4396
    q = np.arange(len(lat))[None]
    d, i = _check_brute([lat], q, 8, exact=True, ks=[1, 2, 6, 7, 8], what="lattice")
    assert (d[0, :, 0] == 0).all()
    rng = np.random.default_rng(1)
    _check_brute([lat, R.lattice(seed=5, integer=integer)], np.sort(rng.integers(0, len(lat), (2, 700)), axis=1), 6, exact=True,
                 what="lattice B=2")


def test_brute_batch_identical_points_and_line():
    same = R.identical(5000)
    q = np.sort(np.random.default_rng(0).integers(0, 5000, (1, 300)), axis=1)
    for K in (1, 6, 8):
        d, i = _check_brute([same], q, K, exact=True, what="identical")
        assert (d == 0).all() and (i[0] == np.arange(K)[None]).all()          # every candidate ties: ids 0 .. K-1
    ln = R.line(4000)
    _check_brute([ln], np.arange(0, 4000, 7)[None], 6, what="line")
    _check_brute([R.offset(20_000), R.clustered(20_000)], np.sort(np.random.default_rng(2).integers(0, 20_000, (2, 512)), axis=1), 6,
                 what="offset / clustered")


@pytest.mark.parametrize("N", [100, 200, 20_000])
def test_brute_batch_window_clamp_at_the_ends(N):
    """the bound's window of 128 index neighbours is clamped into the set for queries within 64 of either end"""
    ends = np.unique(np.clip(np.concatenate([np.arange(0, 72), np.arange(N - 72, N)]), 0, N - 1))
    for order in ("morton", "random"):
        s = R.sheet(N, seed=30, order=order)
        _check_brute([s, s[::-1].copy()], np.stack([ends, ends]), 8, ks=[1, 6, 8], what=f"ends {order}")


@pytest.mark.parametrize("least", [0, 3, 5])
def test_pair_connectivity_on_an_exact_lattice(least):
    radius = 0.1
    sets = [R.aniso_lattice(0), R.aniso_lattice(1)]
    rng = np.random.default_rng(least)
    sample = np.sort(rng.integers(0, len(sets[0]), (2, 600)), axis=1)
    buf = _t(np.stack([np.stack(sets), np.zeros_like(np.stack(sets))], 1))
    got = pair_connectivity(buf[:, 0], _t(sample), K=5, radius=radius, least_edge_num=least)
    assert got.dtype == torch.int32 and got.is_contiguous()
    seen_cut = seen_kept = False
    for b in range(2):
        want, d = R.connectivity64(sets[b], sample[b], 5, radius, least)
        assert np.abs(d - radius ** 2).min() > 1e-3 and (d * 256 == np.round(d * 256)).all()      # exact, far from the threshold
        assert np.array_equal(got[b].cpu().numpy(), want), (b, np.argwhere(got[b].cpu().numpy() != want)[:5])
        seen_cut |= bool((want[:, least:] == -1).any())
        seen_kept |= bool((want >= 0).any())
    assert seen_kept and (seen_cut or least == 5)


@pytest.mark.parametrize("radius", [0.1, 0.02])
def test_pair_connectivity_on_the_morton_sheet(radius):
    N, S, K = 20_000, 512, 5
    sets = [R.sheet(N, seed=40), R.sheet(N, seed=41, noise=1e-3)]
    sample = np.sort(np.random.default_rng(4).integers(0, N, (2, S)), axis=1)
    buf = _t(np.stack([np.stack(sets), np.zeros_like(np.stack(sets))], 1))
    for least in (0, 3, 5):
        got = pair_connectivity(buf[:, 0], _t(sample), K=K, radius=radius, least_edge_num=least).cpu().numpy()
        for b in range(2):
            want, d = R.connectivity64(sets[b], sample[b], K, radius, least)
            near = np.abs(d - radius ** 2) <= 12 * R.U * radius ** 2
            assert near.mean() <= 1e-3                                            # (asserted on the float64 reference alone)
            gap = np.diff(np.concatenate([np.zeros((S, 1)), d], 1), axis=1)      # a float64 near-tie may swap two columns
            sure = ~near & (gap > 12 * R.U * d) & (np.concatenate([gap[:, 1:], np.full((S, 1), 1.0)], 1) > 12 * R.U * d)
            assert sure.mean() > 0.99
            assert np.array_equal(got[b][sure], want[sure])
            assert ((got[b] == -1) == (want == -1))[~near].all()
            if radius == 0.02 and least < 5:
                assert (want == -1).any() and (want[:, least:] >= 0).any()


# ------------------------------------------------------------------ the grid search
def _grid(pts, K, query=None, **kw):
    p = _t(pts)[None]
    q = p if query is None else _t(query)[None]
    r = knn_points(q, p, None, None, K=K, **kw)
    assert r.idx.dtype == torch.int64
    return r.dists[0].cpu().numpy(), r.idx[0].cpu().numpy()


_FAM = {name: (pts, exact) for name, pts, exact in R.families(20_000)}
_REF = {}


def _ref16(name):
    if name not in _REF:
        _REF[name] = R.knn64(_FAM[name][0], _FAM[name][0], 16)
    return _REF[name]


@pytest.mark.parametrize("name", list(_FAM))
def test_grid_search_on_every_family(name):
    """K = 9 and 16 run the 16-register instantiation; the tiny sets hold fewer than K points (its padding)"""
    pts, exact = _FAM[name]
    for K in (1, 6, 8, 9, 16):
        d, i = _grid(pts, K)
        _note("grid", R.check(d, i, pts, pts, K, exact=exact, ref=_ref16(name), what=f"{name} K={K}"))
        if len(pts) < K:
            assert (i[:, len(pts):] == -1).all() and (d[:, len(pts):] == 0).all()


def test_grid_search_batches_return_nn_and_outside_queries():
    rng = np.random.default_rng(4)
    a, b = R.sheet(6000, seed=50), R.clustered(6000, seed=51)
    qa = (rng.normal(size=(2500, 3)) * 1.5 + np.array([0, 0, 3.0])).astype(np.float32)          # queries outside the box too
    qb = (rng.normal(size=(2500, 3)) * 8).astype(np.float32)
    r = knn_points(_t(np.stack([qa, qb])), _t(np.stack([a, b])), None, None, K=9, return_nn=True)
    for s, (q, p) in enumerate(((qa, a), (qb, b))):
        d, i = r.dists[s].cpu().numpy(), r.idx[s].cpu().numpy()
        _note("grid", R.check(d, i, q, p, 9, what=f"B=2 set {s}"))
        assert np.array_equal(r.knn[s].cpu().numpy(), p[i])                   # return_nn = the gather of idx
    lat = R.lattice()
    q = (rng.integers(-4, 21, size=(1500, 3)) / 16.0).astype(np.float32)      # lattice queries on and outside the box: exact
    d, i = _grid(lat, 16, query=q)
    R.check(d, i, q, lat, 16, exact=True, what="lattice, separate queries")
    far = (R.offset(300) + np.float32(3.0)).astype(np.float32)               # every query outside an offset set
    off = R.offset(5000)
    d, i = _grid(off, 6, query=far)
    _note("grid", R.check(d, i, far, off, 6, what="offset, outside queries"))


@pytest.mark.parametrize("name", ["sheet_morton", "clustered", "offset", "lattice", "tiny5", "tiny2"])
def test_distCUDA2_is_the_mean_of_the_three_nearest(name):
    pts = _FAM[name][0]
    got = distCUDA2(_t(pts)).cpu().numpy().astype(np.float64)
    d64 = _ref16(name)[0]
    n = min(3, len(pts) - 1)
    want = d64[:, 1:4].sum(axis=1) / 3.0              # (fewer than four points: the padding's zeros enter the mean, as in the kernel's result)
    err = np.abs(got - want)
    print(f"distCUDA2 {name}: worst {float(np.max(np.divide(err, R.U * want, out=np.zeros_like(err), where=want > 0))):.2f} u (n={n})")
    assert (err <= 8 * R.U * want).all()

