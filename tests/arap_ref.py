"""float64 restatement of the reference's ``estimate_rotation`` + ``cal_arap_error`` (src/geometry_utils.py:50-123) from the
float32 inputs: the reference splat_arap_energy / splat_arap_energy_batch (arap.cal_arap_error, arap_rotations, pair_arap) are
checked against.  Pure numpy (LAPACK's float64 SVD), no GPU, nothing shared with the kernel or with oracle.arap_energy.

Per (sample, frame t >= 1): edges e = p_i - p_j of the K table slots (no edge: 0), S = sum_k w_k e_src e_tgt^T, the reference's
shortcut (one coordinate axis unchanged over all K edges -> S = 0 -> R = I; compared on the FLOAT32 edges, as the kernel and the
reference do), S = U Sigma W^T, R = W U^T with the column of U of the smallest singular value flipped where det <= 0, energy
E(R) = sum_k w_k |e_tgt - R e_src|^2 and its gradient with R held constant.  ``scale = sum_k w_k (|e_tgt| + |e_src|)^2``.

What a float32 kernel may be off by, counted from arap_kernel's operation sequence (u = 2^-24, a = |e_tgt| + |e_src|, each
rounding at most u of its result, FMA contraction only removes roundings):
    e_src, e_tgt = p_i - p_j                 1 rounding each: u |e|
    st = e_tgt - R e_src                     3 products + 2 additions per row (3 sqrt(3) u |e_src| as a vector), the inputs'
                                             roundings (u |e_tgt| + u |e_src|), the subtraction (u |st|, |st| <= a): <= 8 u a
    w |st|^2                                 2 |st| x 8 u a = 16 u a^2, plus 3 squares / 2 additions / the product: 4 u a^2
    e += ..                                  K roundings of partial sums <= the row's energy <= scale
  => |E_kernel - E64(R_kernel)| <= ENERGY_C(K) u scale with ENERGY_C(K) = 20 + K; the scalar the API returns adds one rounding of
     the running sum per atomic addend and one for the division by Nt: (rows + 1) u sum E.
    gt = grad_scale 2 w st                   2 w x 8 u a + 2 products: 10 u m with m = grad_scale 2 w a
    gs = -grad_scale 2 w R^T st              the same + 3 u a for R^T st: 13 u m
    local sums, atomics, the scale by 1/Nt   one rounding per addend of the element (``gcnt``) + 3 spare
  => |grad_kernel - grad64(R_kernel)| <= (GRAD_C + gcnt) u gmag elementwise, GRAD_C = 16, gmag = the summed m of the element.

Measured on an MI355X over every family of tests/test_gpu_arap_reference.py (worst case): energy arithmetic of a row 0.74 u scale,
of the summed scalar 2.3 u scale (bound 20 + K); rotation quality |E64(R_kernel) - E64(R_64)| = 2.53 u scale (a single edge per row;
0.88 on the sheets at K = 5; bound 4); |R R^T - I| = 12.1 u (bound 32); R_kernel against R_64 where sigma_2 > 0.02 sigma_1:
1.6e-6 (bound 1e-4); gradient 0.11 of its bound.  The kernel these tests were first run against took its SVD from a Jacobi
eigen-decomposition of S^T S and failed two of them: rotation quality 16.5 u scale with two nearly collinear edges (K = 2),
|R R^T - I| = 385 u with a single edge per row and 72 u with zero weights (R deviation 5.9e-5); it now runs a one-sided Jacobi
SVD of S itself with a twice-applied Gram-Schmidt step.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
GRAD_C = 16
ROTATION_QUALITY = 4          # |E64(R_kernel) - E64(R_64)| <= 4 u scale: R stored in float32 alone moves the energy by ~3 u scale
ORTHO = 32                    # |R R^T - I| <= 32 u


def ENERGY_C(K: int) -> int:
    return 20 + K


def arap64(nodes, nbr, weight, sample_idx, R=None):
    """``nodes`` [Nt, Nv, 3] float32, ``nbr`` [Nv, K] vertex ids (outside 0..Nv-1: no edge), ``weight`` [Nv, K] or None (1 per edge),
    ``sample_idx`` [S] (duplicates count twice); ``R`` [Nt-1, S, 3, 3]: evaluate energy and gradient with these rotations
    instead of the float64 optimum.  Returns energy / scale / shortcut [Nt-1, S], R [Nt-1, S, 3, 3] (the float64 optimum, always),
    sig [Nt-1, S, 3], grad / gmag [Nt, Nv, 3] (gradient of the UNDIVIDED energy sum; the summed magnitudes 2 w a of the element's
    addends), gcnt [Nt, Nv] (number of addends)."""
    x32 = np.asarray(nodes, np.float32)
    x = x32.astype(np.float64)
    Nt, Nv, _ = x.shape
    tab = np.asarray(nbr).astype(np.int64)
    K = tab.shape[1]
    s = np.asarray(sample_idx, np.int64).reshape(-1)
    S = s.size
    rows = tab[s]
    has = (rows >= 0) & (rows < Nv)
    j = np.where(has, rows, 0)
    w = has.astype(np.float64) if weight is None else np.asarray(weight, np.float32).astype(np.float64)[s]

    def edges(v):
        return np.where(has[..., None], v[s][:, None, :] - v[j], 0)

    Es, Es32 = edges(x[0]), edges(x32[0])
    out = SimpleNamespace(energy=np.zeros((Nt - 1, S)), scale=np.zeros((Nt - 1, S)), shortcut=np.zeros((Nt - 1, S), bool),
                          R=np.zeros((Nt - 1, S, 3, 3)), sig=np.zeros((Nt - 1, S, 3)), grad=np.zeros((Nt, Nv, 3)),
                          gmag=np.zeros((Nt, Nv, 3)), gcnt=np.zeros((Nt, Nv)))
    vi = np.broadcast_to(s[:, None], (S, K))[has]
    vj = j[has]
    for t in range(1, Nt):
        Et, Et32 = edges(x[t]), edges(x32[t])
        assert Es32.dtype == np.float32 and Et32.dtype == np.float32
        Sm = np.einsum("ski,sk,skj->sij", Es, w, Et)
        short = (Es32 == Et32).all(axis=1).any(axis=1)
        Sm[short] = 0
        Um, sig, Wt = np.linalg.svd(Sm)
        W = np.transpose(Wt, (0, 2, 1))
        R64 = W @ np.transpose(Um, (0, 2, 1))
        flip = np.flatnonzero(np.linalg.det(R64) <= 0)
        if flip.size:
            Uf = Um[flip].copy()
            Uf[np.arange(flip.size), :, np.argmin(sig[flip], axis=1)] *= -1
            R64[flip] = W[flip] @ np.transpose(Uf, (0, 2, 1))
        Ru = R64 if R is None else np.asarray(R[t - 1]).astype(np.float64)
        st = Et - np.einsum("sij,skj->ski", Ru, Es)
        a = np.linalg.norm(Et, axis=2) + np.linalg.norm(Es, axis=2)
        out.energy[t - 1] = (w * np.square(st).sum(-1)).sum(1)
        out.scale[t - 1] = (w * np.square(a)).sum(1)
        out.shortcut[t - 1], out.R[t - 1], out.sig[t - 1] = short, R64, sig
        gt = (2.0 * w[..., None] * st)[has]
        gs = (-2.0 * w[..., None] * np.einsum("sji,skj->ski", Ru, st))[has]
        m = np.broadcast_to((2.0 * np.abs(w) * a)[..., None], st.shape)[has]
        for f, g in ((t, gt), (0, gs)):
            np.add.at(out.grad[f], vi, g)
            np.add.at(out.grad[f], vj, -g)
            for v in (vi, vj):
                np.add.at(out.gmag[f], v, m)
                np.add.at(out.gcnt[f], v, 1.0)
    return out


def expand_rows(nbr_rows, sample_idx, Nv: int) -> np.ndarray:
    """[Nv, K] table (-1 elsewhere) from the compact [S, K] rows of the sampled vertices (pair_connectivity's result); a vertex
    sampled twice must carry the same row twice"""
    rows = np.asarray(nbr_rows).astype(np.int64)
    s = np.asarray(sample_idx, np.int64)
    tab = np.full((Nv, rows.shape[1]), -1, np.int64)
    tab[s] = rows
    assert np.array_equal(tab[s], rows), "a vertex sampled twice has two different neighbour rows"
    return tab
