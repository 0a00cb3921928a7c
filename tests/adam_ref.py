"""float64 restatement of torch.optim.Adam (no weight decay, no amsgrad): the reference the Adam kernels behind optim.FlatAdam /
optim.OwnerShardedAdam (splat_adam_step, splat_adam_step_pattern) are checked against.

The per-element learning rate is built here from the bucket's slices and the groups' rates -- a PatternLR group's phase counted
from the group's first element -- and NOT through optim.lr_segments or OwnerShardedAdam._segments: this is the independent
statement those are checked against.  Pure numpy, no GPU.

The hyper-parameters go in as the kernels receive them through the C ABI, as float32 (``f32``): 1 - float32(0.999) is 1.3e-5
relative off 0.001, far above any rounding, and a float32 Adam asked for beta2 = 0.999 runs with that value.
"""
from __future__ import annotations

import numpy as np

from splatter_a_video_amd.optim import PatternLR

U = 2.0 ** -24          # float32 unit roundoff: one rounding is off by at most U of its exact result


def f32(x: float) -> float:
    """``x`` as the float32 the C ABI carries, back in float64"""
    return float(np.float32(x))


def rate_map(slices, lrs, total: int) -> np.ndarray:
    """per-element learning rate (float64) of a flat buffer of ``total`` floats laid out by ``slices`` ({name: (a, b)}); a
    ``PatternLR`` group gives the first ``head`` of every ``period`` elements, counted from the group's start, ``head_lr``;
    elements of no slice (the bucket's padding) get 0"""
    out = np.zeros(total, dtype=np.float64)
    for name, (a, b) in slices.items():
        r = lrs[name]
        if isinstance(r, PatternLR):
            k = np.arange(b - a)
            out[a:b] = np.where(k % r.period < r.head, r.head_lr, r.lr)
        else:
            out[a:b] = float(r)
    return out


class Adam64:
    """``torch.optim.Adam`` step by step in float64 on a flat buffer, with a per-element learning rate (``rate_map``), and beside
    it a first-order bound on how far a float32 implementation of the same steps can be from it (``check``).

    The bound counts the roundings of one float32 step, each at most U of the value it rounds, and carries the earlier steps'
    errors along (the moments' through their decay):
        m = b1 m + (1 - b1) (g s)          4 roundings of |b1 m| + |(1 - b1) g s|
        v = b2 v + (1 - b2) (g s)^2        6 of b2 v + (1 - b2) (g s)^2   (g s enters twice)
        dp = (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
                                           8 of |dp| (lr / bc1, 1 / sqrt(bc2), sqrt, *, + eps, *, /, one spare), plus what the
                                           errors of m and v make of it: (lr / bc1) e_m / denom and |dp| e_v / (2 v)
        p = p + dp                         1 of |p|, plus the error of dp"""

    def __init__(self, param, betas=(0.9, 0.999), eps: float = 1e-15):
        self.p = np.array(param, dtype=np.float64)
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.b1, self.b2 = float(betas[0]), float(betas[1])
        self.eps = float(eps)
        self.t = 0
        self.e_p = np.zeros_like(self.p)
        self.e_m = np.zeros_like(self.p)
        self.e_v = np.zeros_like(self.p)

    def step(self, grad, lr, grad_scale: float = 1.0) -> None:
        """``grad_scale`` multiplies the gradient before both moments; ``lr``: a number or one rate per element"""
        self.t += 1
        b1, b2 = self.b1, self.b2
        g = np.asarray(grad, dtype=np.float64) * float(grad_scale)
        m_old, m_new = b1 * self.m, (1.0 - b1) * g
        v_old, v_new = b2 * self.v, (1.0 - b2) * g * g
        self.m = m_old + m_new
        self.v = v_old + v_new
        self.e_m = b1 * self.e_m + 4 * U * (np.abs(m_old) + np.abs(m_new))
        self.e_v = b2 * self.e_v + 6 * U * (v_old + v_new)
        bc1 = 1.0 - b1 ** self.t
        bc2 = 1.0 - b2 ** self.t
        ss = np.asarray(lr, dtype=np.float64) / bc1
        denom = np.sqrt(self.v) / np.sqrt(bc2) + self.eps
        dp = -ss * self.m / denom
        self.p = self.p + dp
        rel_v = np.divide(self.e_v, 2.0 * self.v, out=np.zeros_like(self.v), where=self.v > 0)   # v = 0: m = 0, dp = 0
        self.e_p = self.e_p + U * np.abs(self.p) + np.abs(dp) * (8 * U + rel_v) + np.abs(ss) * self.e_m / denom

    def check(self, p, m=None, v=None, what: str = "") -> None:
        """a float32 implementation's parameters (and moments) within the bound, element by element"""
        for name, got, want, e in (("param", p, self.p, self.e_p), ("exp_avg", m, self.m, self.e_m),
                                   ("exp_avg_sq", v, self.v, self.e_v)):
            if got is None:
                continue
            got = np.asarray(got, dtype=np.float64)
            assert got.shape == want.shape, (what, name, got.shape, want.shape)
            err = np.abs(got - want)
            bad = np.flatnonzero(~(err <= e))          # (a NaN is out of bounds too)
            if bad.size:
                i = int(bad[0])
                raise AssertionError(f"{what} {name}: {bad.size} of {got.size} elements beyond float32 rounding after {self.t} "
                                     f"steps; first at {i}: got {got[i]!r}, float64 {want[i]!r}, bound {e[i]!r}")
