"""tests/knn_ref.py itself: the float64 search against the C oracle, a float32 numpy model of the kernels' arithmetic accepted on
every input family (bit-equal on the exact ones), and the mistakes ``check`` has to reject."""
import numpy as np
import pytest

import knn_ref as R


def test_knn64_is_the_oracle_search(oracle_mod):
    pts = R.cloud(3000)
    d, i = R.knn64(pts[:700], pts, 7)
    od, oi = oracle_mod.knn_points(pts[:700], pts, 7)
    assert np.array_equal(i, oi)                                  # (a normal cloud has no near-ties at float32's resolution)
    np.testing.assert_allclose(od, d, rtol=6 * R.U, atol=0)
    lat = R.lattice()
    d, i = R.knn64(lat[:500], lat, 9)                             # exact distances: the oracle's float32 search is the same search
    od, oi = oracle_mod.knn_points(lat[:500], lat, 9)
    assert np.array_equal(i, oi) and np.array_equal(d, od.astype(np.float64))
    d, i = R.knn64(pts[:4], pts[:3], 5)                           # fewer points than K: 0 / -1 padding
    assert (i[:, 3:] == -1).all() and (d[:, 3:] == 0).all() and (np.sort(i[:, :3], axis=1) == np.arange(3)).all()


def test_knn64_orders_ties_by_index_across_chunks():
    pts = R.identical(5000)
    d, i = R.knn64(pts[:40], pts, 6)
    assert (d == 0).all() and (i == np.arange(6)[None]).all()
    big = np.concatenate([R.cloud(2_100_000 // 50), R.cloud(10)])          # rows split over several chunks
    d1, i1 = R.knn64(big[:120], big, 4)
    d2 = R._dist64(big[:120].astype(np.float64), big.astype(np.float64))
    assert np.array_equal(i1, np.argsort(d2, axis=1, kind="stable")[:, :4])


def test_float32_model_passes_on_every_family():
    worst = 0.0
    for name, pts, exact in R.families(2500):
        rng = np.random.default_rng(len(pts))
        q = pts[np.sort(rng.integers(0, len(pts), 200))]
        for K in (1, 6, 16):
            d, i = R.model32(q, pts, K)
            worst = max(worst, R.check(d, i, q, pts, K, exact=exact, what=f"{name} K={K}"))
    print(f"float32 model: worst distance error {worst:.2f} u")
    assert worst <= 6


def test_connectivity64_cuts_past_least_edge_num():
    lat = R.aniso_lattice()
    sample = np.arange(0, len(lat), 7)
    for least in (0, 3, 5):
        nbr, d = R.connectivity64(lat, sample, K=5, radius=0.1, least_edge_num=least)
        assert np.abs(d - 0.01).min() > 1e-3 and ((d * 256) == np.round(d * 256)).all()
        want_cut = d >= 0.01
        want_cut[:, :least] = False
        assert ((nbr == -1) == want_cut).all()
        assert (nbr[~want_cut] != sample[:, None].repeat(5, 1)[~want_cut]).all()          # the vertex itself was dropped
    cut = R.connectivity64(lat, sample, 5, 0.1, 0)[0] == -1
    assert cut.any() and (~cut).any()


@pytest.fixture(scope="module")
def good():
    pts = R.cloud(2000)
    q = pts[:50]
    d, i = R.model32(q, pts, 6)
    R.check(d, i, q, pts, 6)
    return pts, q, d, i


def _rejects(rule, d, i, q, pts, K=6, exact=False):
    with pytest.raises(AssertionError, match=f"rule {rule}"):
        R.check(d, i, q, pts, K, exact=exact)


def test_check_rejects_a_neighbour_replaced_by_the_next(good):
    pts, q, d, i = good
    d7, i7 = R.model32(q, pts, 7)
    d, i = d.copy(), i.copy()
    d[9, 5], i[9, 5] = d7[9, 6], i7[9, 6]                         # row 9 holds the 7th in place of the 6th
    _rejects(3, d, i, q, pts)
    d, i = good[2].copy(), good[3].copy()
    d[9, 2:5], i[9, 2:5] = d[9, 3:6].copy(), i[9, 3:6].copy()     # an inner neighbour missing, the 7th appended
    d[9, 5], i[9, 5] = d7[9, 6], i7[9, 6]
    _rejects(3, d, i, q, pts)


def test_check_rejects_a_swapped_exact_tie():
    lat = R.lattice()
    q = lat[:30]
    d, i = R.model32(q, lat, 6)
    R.check(d, i, q, lat, 6, exact=True)
    r, c = np.argwhere(d[:, 1:] == d[:, :-1])[0]
    i = i.copy()
    i[r, c], i[r, c + 1] = i[r, c + 1], i[r, c]
    _rejects(4, d, i, q, lat)
    # a tie cut at the K-th place towards the larger index: nothing inside the row shows it, only the exact comparison
    d7, i7 = R.model32(q, lat, 7)
    r = int(np.flatnonzero(d7[:, 5] == d7[:, 6])[0])
    i = R.model32(q, lat, 6)[1]
    i[r, 5] = i7[r, 6]
    R.check(d, i, q, lat, 6)
    _rejects(5, d, i, q, lat, exact=True)


def test_check_rejects_a_duplicate_id_bad_padding_and_a_wrong_distance(good):
    pts, q, d, i = good
    i2 = i.copy(); i2[3, 4] = i2[3, 3]
    _rejects(1, d, i2, q, pts)
    i2 = i.copy(); i2[3, 4] = len(pts)
    _rejects(1, d, i2, q, pts)
    d2 = d.copy(); d2[7, 3] *= np.float32(1 + 1e-6)
    _rejects(2, d2, i, q, pts)
    d2 = d.copy(); d2[7, 3] *= np.float32(1 - 1e-6)
    _rejects(2, d2, i, q, pts)
    dt, it = R.model32(q[:5], pts[:4], 6)                         # padding columns
    R.check(dt, it, q[:5], pts[:4], 6)
    it2 = it.copy(); it2[0, 5] = 0
    _rejects(1, dt, it2, q[:5], pts[:4])
