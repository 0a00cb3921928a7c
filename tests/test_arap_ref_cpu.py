"""tests/arap_ref.py itself: the float64 restatement pinned to oracle.arap_energy (numpy float32 edges, LAPACK SVD; itself pinned
to the reference's own vectors in test_arap_cpu.py) on the golden case, and its degenerate rows."""
import os

import numpy as np
import pytest

import arap_ref as A

G = os.path.join(os.path.dirname(__file__), "golden", "arap_2000.npz")


@pytest.mark.parametrize("tag", ["unit", "weighted"])
def test_arap64_matches_the_oracle(oracle_mod, tag):
    g = dict(np.load(G))
    Nt, Nv, K = g["nodes"].shape[0], g["nodes"].shape[1], int(g["K"])
    nbr = np.full((Nv, K), -1, np.int32)
    nbr[g["ii"], g["nn"]] = g["jj"]
    w = None if tag == "unit" else g["weight"]
    sidx = g[f"{tag}_sample_idx"]
    e, grad, rots = oracle_mod.arap_energy(g["nodes"], nbr, w, sidx)
    r = A.arap64(g["nodes"], nbr, w, sidx)
    assert abs(r.energy.sum() / Nt - float(e)) < 2e-6 * float(e)
    assert abs(r.energy.sum() / Nt - float(g[f"{tag}_error"])) < 2e-5 * float(g[f"{tag}_error"])
    np.testing.assert_allclose(r.R, rots, rtol=0, atol=2e-6)                      # (the oracle stores float32 rotations)
    np.testing.assert_allclose(r.grad / Nt, grad, rtol=0, atol=2e-6 * float(np.abs(grad).max()))
    assert r.shortcut[2].all() and not r.shortcut[0].any()                         # frame 3 of the golden case moves in the xy plane only
    assert np.abs(r.R[2] - np.eye(3)).max() == 0
    assert (np.linalg.det(r.R) > 0.999999).all() and (r.scale >= r.energy).all()
    # evaluating with given rotations: the optimum's own reproduce it; any other rotation has a higher energy
    again = A.arap64(g["nodes"], nbr, w, sidx, R=r.R)
    assert np.array_equal(again.energy, r.energy) and np.array_equal(again.grad, r.grad)
    c, s = np.cos(0.01), np.sin(0.01)
    off = r.R @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    worse = A.arap64(g["nodes"], nbr, w, sidx, R=off)
    assert (worse.energy[0] > r.energy[0]).all()
    # translation invariance
    assert np.abs(r.grad.sum(axis=1)).max() < 1e-9 * np.abs(r.grad).max() * Nv
    assert r.gcnt[0].sum() == r.gcnt[1:].sum() and (r.gmag >= np.abs(r.grad) * (1 - 1e-12)).all()


def test_arap64_degenerate_rows():
    rng = np.random.default_rng(0)
    src = rng.normal(size=(12, 3)).astype(np.float32)
    tgt = (src @ np.array([[0.8, -0.6, 0], [0.6, 0.8, 0], [0, 0, 1.0]]).T + 0.01 * rng.normal(size=src.shape)).astype(np.float32)
    tgt[4:8] = src[4:8]                                          # vertices 4..7 do not move
    nbr = np.full((12, 3), -1)
    nbr[0] = [1, 2, 3]                                           # generic
    nbr[1, 1] = 2                                                # one edge
    nbr[4] = [5, 6, 7]                                           # source == target
    nbr[9] = [99, -5, 12]                                        # ids outside the set: no edge
    r = A.arap64(np.stack([src, tgt]), nbr, None, np.array([0, 1, 4, 8, 9, 0]))
    assert r.shortcut[0].tolist() == [False, False, True, True, True, False]
    assert (r.energy[0, 2:5] == 0).all() and (np.abs(r.R[0, 2:5] - np.eye(3)) == 0).all()
    s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
    e = np.linalg.norm(t64[1] - t64[2]) - np.linalg.norm(s64[1] - s64[2])     # one edge: the rotation aligns it, the length change stays
    assert abs(r.energy[0, 1] - e * e) < 1e-12
    assert r.energy[0, 0] == r.energy[0, 5] and r.gcnt[0, 0] == 6 and r.gcnt[0, 9] == 0 and (r.grad[:, 8:] == 0).all()
    assert (A.expand_rows([[1, 2], [3, 4], [1, 2]], [5, 0, 5], 7)[[0, 5, 6]] == [[3, 4], [1, 2], [-1, -1]]).all()
    with pytest.raises(AssertionError):
        A.expand_rows([[1, 2], [3, 4]], [5, 5], 7)
