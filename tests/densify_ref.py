"""References and seeded cases for the densification kernels (csrc/densify.hip, splatter_a_video_amd/densify.py): pure numpy,
importable without a GPU.  tests/test_densify_ref_cpu.py holds the references to the C oracle and to published vectors,
tests/test_gpu_densify_reference.py and tests/test_gpu_train_step_densify.py hold the kernels to the references.

DECISIONS (``masks_ref``).  The inputs are the float32 values the kernel reads, the arithmetic is float64, the thresholds are
the float32 values the kernel compares with (``thresholds``: the arguments rounded to float32, the two products rounded once
more).  Every comparison returns its float64 distance to the threshold relative to the larger of the two compared magnitudes.
A row takes part in a decision's comparison unless one of THAT decision's comparisons is within MULT * 2^-24 of its threshold
(MULT = 16 as tests/geometry_ref.py: expf / the sigmoid at about 2 ulp = 4 * 2^-24, one divide, the threshold's product --
under 8 * 2^-24, doubled).  ``max_radii2D > size_threshold`` compares two float32 inputs: it has no rounding and no margin.
Rows of the tie stratum are compared whatever their margin: each of their comparisons is exact in float32 or clear.

CHILDREN (``children_ref`` / ``children_f32``) and NORMALS (``normals_ref`` / ``normals_f32``): float64 references with
per-element bars derived from the operation count (below, at K_POS / K_SCL / K_BM), and float32 numpy restatements of the
kernel's arithmetic that must stay inside the same bars on the CPU (profiles/densify_reference_cpu_float32.json).
"""
import numpy as np

EPS32 = 2.0 ** -24
MULT = 16.0
EXCLUDE_CAP = 0.01
F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------------
# bars of the children, in units of EPS32 = 2^-24 (half an ulp, relative).  Device expf / logf / sinf / cosf are taken at
# <= 2 ulp = 4 EPS32, sqrtf and the divide at <= 1 ulp = 2 EPS32, a multiply or an add at 1 EPS32.
#
# SCALE  b = s - log(0.8 n), the kernel evaluates logf(expf(s) / (0.8f * n)):
#   expf(s): 4 relative = 4 absolute in the logarithm; 0.8f (0.25) and its product with n (1): 1.25; the divide: 2; all
#   absolute in the logarithm: 7.25.  logf itself: 4 relative to |b|.  7.25 + 4 |b| <= 8 (1 + |b|):
K_SCL = 8.0
#
# POSITION  a_k = sum_j R_kj m_j + p_k, m_j = z_j exp(s_j), R from q / |q|:
#   m_j: expf 4 + multiply 1 = 5, relative to |m_j|.
#   q / |q|: four squares (1 each) and three adds (1 each) leave <= 4 on the sum of squares = 2 on the norm, sqrtf 2, the
#   divide 2: every unit component within 6 of its value, 4 of them common to the four components.
#   R_kj off the diagonal = 2 (x y -+ r z): each product 6 + 6 + 1 = 13 relative to |x y| resp. |r z|, the subtraction 1.
#   On the diagonal 1 - 2 (x^2 + z^2): 13 on each square, 2 adds.
#   The errors of the entries are therefore ABSOLUTE: <= 13 * 2 (|x y| + |r z|) + 1 <= 14 (2 |x y| + 2 |r z| <= |q|^2 = 1),
#   NOT relative to |R_kj|, which the subtraction may have cancelled.  The bar's magnitude has to carry the entry's operands,
#   not its value: sum_j A_kj |m_j| with A_kj = 2 (|x y| + |r z|) off the diagonal and 1 + 2 (x^2 + z^2) - the operands of the
#   expression that forms R_kj - in place of |R_kj|.  A_kj >= |R_kj| everywhere and A_kj = |R_kj| wherever nothing cancels
#   (``children_ref`` returns both magnitudes; the float32 restatement on the CPU shows the |R_kj| form out of reach of ANY
#   float32 evaluation: tests/test_densify_ref_cpu.py::test_position_bar_needs_the_entries_operands).
#   Per term: (14 + 5 + 1 [the product]) A_kj |m_j|; the three adds of the sum: 3 relative to the partial sums, each below the
#   magnitude.  23 in all, rounded up to
K_POS = 24.0
#
# NORMALS  z = r cos(a) (sin for the second), r = sqrt(-2 log u), a = float32(2 pi) * u rounded to float32 (restated exactly):
#   logf 4 relative to |log u| = 2 on r, sqrtf 2, cosf / sinf 4 absolute (|.| <= 1), the product 1: 9 r, rounded up to
K_BM = 12.0           # |z - z_ref| <= K_BM * EPS32 * (1 + r)


# ---------------------------------------------------------------------------------------------------------------------
# decisions
# ---------------------------------------------------------------------------------------------------------------------
def thresholds(grad_threshold, percent_dense, cameras_extent, min_opacity, size_threshold):
    """the float32 values splat_densify_masks compares with"""
    return dict(grad=F32(grad_threshold), dense=F32(F32(percent_dense) * F32(cameras_extent)),
                big_ws=F32(F32(0.1) * F32(cameras_extent)), min_opacity=F32(min_opacity), size=F32(size_threshold))


def _rel(x, t):
    x = np.asarray(x, np.float64)
    t = np.float64(t)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.abs(x - t) / np.maximum(np.abs(x), np.abs(t))
    d = np.where(np.isinf(x), np.inf, d)
    return np.where(np.isnan(d), 0.0, d)          # 0 against 0: on the threshold


def masks_ref(accum, denom, max_radii2D, scaling_raw, opacity_raw, th, grad_slack=0.0):
    """float64 decisions of generate_clone_mask / generate_split_mask / the prune filter (reference:
    src/pointrix/optimizer/atlas_gs_optimizer.py:199-253, :363-375).  -> dict(clone, split, prune [N] bool, dist {comparison:
    [N] relative distance}, clear {decision: [N] bool}).  ``grad_slack`` widens the margin of the gradient comparisons: the
    relative tolerance under which the other side's pos_gradient_accum was itself compared, when it is not the one given here"""
    for a in (accum, denom, max_radii2D, scaling_raw, opacity_raw):
        assert np.asarray(a).dtype == np.float32
    acc = np.asarray(accum, np.float64).reshape(-1)
    den = np.asarray(denom, np.float64).reshape(-1)
    mr = np.asarray(max_radii2D, np.float64).reshape(-1)
    sc = np.asarray(scaling_raw, np.float64).reshape(-1, 3)
    op = np.asarray(opacity_raw, np.float64).reshape(-1)
    t = {k: np.float64(v) for k, v in th.items()}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g = acc / den
        g = np.where(np.isnan(g), 0.0, g)             # never visible: 0 / 0; x / 0 stays inf
        smax = np.exp(sc.max(1))
        opac = 1.0 / (1.0 + np.exp(-op))
    clone = (np.abs(g) >= t["grad"]) & (smax <= t["dense"])
    split = (g >= t["grad"]) & (smax > t["dense"])
    sized = t["size"] > 0
    prune = (opac < t["min_opacity"]) | (sized & ((mr > t["size"]) | (smax > t["big_ws"])))
    dist = dict(grad_abs=_rel(np.abs(g), t["grad"]), grad=_rel(g, t["grad"]), dense=_rel(smax, t["dense"]),
                big_ws=_rel(smax, t["big_ws"]), min_opacity=_rel(opac, t["min_opacity"]), size=_rel(mr, t["size"]))
    m = MULT * EPS32
    mg = m + grad_slack
    clear = dict(clone=(dist["grad_abs"] > mg) & (dist["dense"] > m), split=(dist["grad"] > mg) & (dist["dense"] > m),
                 prune=(dist["min_opacity"] > m) & ((dist["big_ws"] > m) | ~sized))
    return dict(clone=clone, split=split, prune=prune, dist=dist, clear=clear, g=g, smax=smax, opac=opac)


def mismatch_margins(got, ref):
    """for a (clone, split, prune) triple of the code under test: {decision: (rows that differ, rows that differ although
    the reference is clear there)}"""
    out = {}
    for k, a in zip(("clone", "split", "prune"), got):
        bad = np.asarray(a, bool).reshape(-1) != ref[k]
        out[k] = (np.flatnonzero(bad), np.flatnonzero(bad & ref["clear"][k]))
    return out


MASK_N = (1, 255, 256, 257, 70_001)
# name -> (densify_grad_threshold, percent_dense, cameras_extent, min_opacity, size_threshold)
MASK_PARAMS = {
    "scale": (2e-4, 0.01, 3.0, 0.005, 20.0),       # test_masks_match_oracle_at_scale
    "ties": (2e-4, 0.5, 2.0, 0.5, 20.0),           # dense = 1 = exp(0), min_opacity = 0.5 = sigmoid(0)
    "nosize": (2e-4, 0.01, 3.0, 0.005, 0.0),       # size_threshold = 0: prune by opacity alone
}
STRATA = ("control", "near", "tie", "special")


def _deliberate_rows(th):
    """rows (accum, denom, max_radii2D, scaling[3], opacity, stratum) placed on, next to and far beyond the thresholds"""
    grad, dense, big, mino, size = (float(th[k]) for k in ("grad", "dense", "big_ws", "min_opacity", "size"))
    lo = min(np.log(dense), np.log(big)) - 6.0                 # a scale clearly under both world-size thresholds
    hi_g = lambda d: F32(4.0 * grad * d)                       # a gradient clearly over its threshold
    logit = lambda p: float(np.log(p / (1.0 - p)))
    rows = []
    add = lambda acc, den, mr, sc, op, s: rows.append((F32(acc), F32(den), F32(mr), np.asarray(sc, np.float32), F32(op), s))
    # ties: every float32 intermediate exact (accum / 1, expf(0) = 1, 1 / (1 + expf(-0)) = 0.5, two inputs)
    add(th["grad"], 1.0, 1.0, (0.0, 0.0, 0.0), 4.0, "tie")              # >= grad; smax = 1 (= dense under "ties": clone, no split)
    add(th["grad"], 1.0, 1.0, (3.0, lo, 3.0), 4.0, "tie")               # >= grad with a clearly large scale: split
    add(hi_g(1), 1.0, 0.0, (lo, lo, lo), 0.0, "tie")                    # opacity 0.5 (= min_opacity under "ties": not pruned)
    add(hi_g(1), 1.0, th["size"], (lo, lo, lo), 5.0, "tie")             # max_radii2D = size_threshold: not pruned
    # near: relative distance 1e-4 on either side of each threshold, everything else clear
    for sgn in (-1.0, 1.0):
        f = 1.0 + sgn * 1e-4
        for den in (1.0, 3.0):
            add(grad * f * den, den, 1.0, (lo, lo - 1, lo - 2), 4.0, "near")                       # clone decided by grad
            add(grad * f * den, den, 1.0, (np.log(dense) + 1.0, lo, lo), 4.0, "near")              # split decided by grad
        add(hi_g(2), 2.0, 1.0, (lo, np.log(dense * f), lo), 4.0, "near")                            # clone / split by dense
        add(hi_g(2), 2.0, 1.0, (np.log(big * f), lo, lo), 4.0, "near")                              # prune by big_ws
        add(hi_g(2), 2.0, 1.0, (lo, lo, lo), logit(mino * f), "near")                               # prune by opacity
        add(hi_g(2), 2.0, size * f if size > 0 else (1.0 + sgn), (lo, lo, lo), 4.0, "near")         # prune by radius
    # special values
    add(0.0, 0.0, 0.0, (lo, lo, lo), 4.0, "special")                    # 0 / 0 -> 0: neither clone nor split
    add(0.0, 0.0, 0.0, (np.log(dense) + 1.0, lo, lo), 4.0, "special")
    add(1e-3, 0.0, 0.0, (lo, lo, lo), 4.0, "special")                   # x / 0 -> inf: clone
    add(1e-3, 0.0, 0.0, (np.log(dense) + 1.0, lo, lo), 4.0, "special")  #               split
    add(-1e-3, 0.0, 0.0, (lo, lo, lo), 4.0, "special")                  # -inf: |g| clones, g does not split
    add(-1e-3, 0.0, 0.0, (np.log(dense) + 1.0, lo, lo), 4.0, "special")
    add(-4.0 * grad, 1.0, 0.0, (lo, lo, lo), 4.0, "special")            # a negative mean: clone by |g|
    add(-4.0 * grad, 1.0, 0.0, (np.log(dense) + 1.0, lo, lo), 4.0, "special")
    add(hi_g(2), 2.0, 1.0, (100.0, 100.0, 100.0), 4.0, "special")       # exp overflows: inf
    add(hi_g(2), 2.0, 1.0, (-100.0, 100.0, -100.0), 4.0, "special")
    add(hi_g(2), 2.0, 1.0, (-100.0, -100.0, -100.0), 4.0, "special")    # exp underflows: 0
    add(hi_g(2), 2.0, 1000.0, (lo, lo, lo), 4.0, "special")             # a huge radius: pruned unless size_threshold = 0
    add(hi_g(2), 2.0, 1.0, (np.log(big) + 2.0, lo, lo), 4.0, "special")  # a huge scale: pruned unless size_threshold = 0
    add(hi_g(2), 2.0, 1000.0, (np.log(big) + 2.0, lo, lo), -30.0, "special")   # transparent: pruned either way
    add(hi_g(2), 2.0, 1.0, (lo, lo, lo), 30.0, "special")               # sigmoid saturates at 1
    return rows


def mask_case(N, params, seed=0):
    """one case: every stratum mixed into N rows (the deliberate rows at seeded places, the first and the last row among them;
    N = 1 holds the first tie row).  -> dict(accum, denom, max_radii2D [N], scaling_raw [N,3], opacity_raw [N,1], args, th,
    stratum [N] index into STRATA, ref)"""
    args = MASK_PARAMS[params]
    th = thresholds(*args)
    rng = np.random.default_rng([seed, N, sorted(MASK_PARAMS).index(params)])
    # control: the distributions of test_masks_match_oracle_at_scale
    acc = (np.abs(rng.normal(size=N)) * 1e-3).astype(np.float32)
    den = rng.integers(0, 5, size=N).astype(np.float32)
    mr = rng.integers(0, 40, size=N).astype(np.float32)
    sc = rng.normal(-4, 1.5, size=(N, 3)).astype(np.float32)
    op = rng.normal(-2, 3, size=(N, 1)).astype(np.float32)
    stratum = np.zeros(N, np.int8)
    rows = _deliberate_rows(th)
    place = rng.permutation(N)
    if N >= 2:                                           # the first and the last row of the launch are deliberate rows
        place = np.concatenate([[0, N - 1], place[(place != 0) & (place != N - 1)]])
    for k, (a, d, m, s, o, name) in enumerate(rows[:N]):
        i = place[k]
        acc[i], den[i], mr[i], sc[i], op[i, 0], stratum[i] = a, d, m, s, o, STRATA.index(name)
    ref = masks_ref(acc, den, mr, sc, op, th)
    return dict(id=f"{params}.N{N}", N=N, accum=acc, denom=den, max_radii2D=mr, scaling_raw=sc, opacity_raw=op, args=args, th=th,
                stratum=stratum, ref=ref)


def compared_rows(case, decision):
    """rows of ``case`` on which ``decision`` is compared: the clear ones and the whole tie stratum"""
    return case["ref"]["clear"][decision] | (case["stratum"] == STRATA.index("tie"))


def excluded_share(case, decision):
    return float((~compared_rows(case, decision)).sum()) / case["N"]


# ---------------------------------------------------------------------------------------------------------------------
# statistics: accumulate_frame / update restated in float32 numpy, in the kernel's operation order
# ---------------------------------------------------------------------------------------------------------------------
class StatsRef:
    """the state of densify.DensifyState as numpy arrays; ``accum64`` follows pos_gradient_accum in float64 (from the float32
    viewspace_grad both sides hold bit for bit)"""

    def __init__(self, N, sentinel=None):
        self.N = N
        z = lambda dt, *s: np.zeros((N,) + s, dt)
        self.max_radii2D, self.pos_gradient_accum, self.denom = z(np.float32), z(np.float32), z(np.float32)
        self.viewspace_grad, self.visibility, self.radii = z(np.float32, 2), z(np.uint8), z(np.int32)
        if sentinel is not None:
            for k, v in sentinel.items():
                getattr(self, k)[...] = v.reshape(getattr(self, k).shape)
        self.accum64 = self.pos_gradient_accum.astype(np.float64)

    def begin_batch(self):
        self.viewspace_grad[...] = 0
        self.visibility[...] = 0
        self.radii[...] = 0

    def accumulate_frame(self, radius, tap, scale=(1.0, 1.0)):
        if tap is not None:
            prod = tap * np.array([F32(scale[0]), F32(scale[1])], np.float32)     # the rounded product first
            assert prod.dtype == np.float32
            self.viewspace_grad += prod                                            # then the add
        self.visibility[radius > 0] = 1
        np.maximum(self.radii, radius, out=self.radii)

    def update(self):
        v = self.visibility != 0
        self.max_radii2D[v] = np.maximum(self.max_radii2D[v], self.radii[v].astype(np.float32))
        g = self.viewspace_grad[v]
        self.pos_gradient_accum[v] += np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
        g = g.astype(np.float64)
        self.accum64[v] += np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
        self.denom[v] += F32(1.0)

    def prune_postprocess(self, valid):
        valid = np.asarray(valid, bool)
        self.max_radii2D, self.pos_gradient_accum, self.denom = self.max_radii2D[valid], self.pos_gradient_accum[valid], self.denom[valid]
        self.accum64 = self.accum64[valid]
        self.N = int(valid.sum())
        self.viewspace_grad, self.visibility = np.zeros((self.N, 2), np.float32), np.zeros(self.N, np.uint8)
        self.radii = np.zeros(self.N, np.int32)


STATS_SCALE = (0.5 * 853, 0.5 * 479)


def stats_frames(N, F, seed, taps=True):
    """F frames of (radius int32 [N] with values <= 0 among them, tap float32 [N,2] of magnitude 1e-12 .. 1e12 or None)"""
    rng = np.random.default_rng([seed, N, F])
    out = []
    for _ in range(F):
        radius = rng.integers(-3, 9, size=N).astype(np.int32)
        radius[rng.random(N) < 0.3] = 0
        tap = None
        if taps:
            tap = (rng.choice([-1.0, 1.0], size=(N, 2)) * 10.0 ** rng.uniform(-12, 12, size=(N, 2))).astype(np.float32)
        out.append((radius, tap))
    return out


def stats_sentinels(N, seed):
    """a state no kernel wrote: update() must leave the rows it does not see bit for bit"""
    rng = np.random.default_rng([seed, N, 77])
    return dict(max_radii2D=rng.integers(0, 50, size=N).astype(np.float32), pos_gradient_accum=rng.uniform(0, 5, size=N).astype(np.float32),
                denom=rng.integers(0, 9, size=N).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# the counter-based generator: Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3; SC'11)
# ---------------------------------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ten rounds on Python integers: ctr = (c0, c1, c2, c3), key = (k0, k1) -> four 32-bit words"""
    c0, c1, c2, c3 = (int(c) & _MASK for c in ctr)
    k0, k1 = (int(k) & _MASK for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def philox4x32_10_np(c0, c1, c2, c3, k0, k1):
    """the same on uint64 arrays holding 32-bit words (a 32 x 32 bit product fits); checked against the integer version"""
    u = lambda a: np.asarray(a, np.uint64)
    c0, c1, c2, c3 = np.broadcast_arrays(u(c0), u(c1), u(c2), u(c3))
    k0, k1, mask, s32 = np.uint64(int(k0) & _MASK), np.uint64(int(k1) & _MASK), np.uint64(_MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(_W0)) & mask, (k1 + np.uint64(_W1)) & mask
    return c0, c1, c2, c3


U01_ONE, U01_MIN = 0xFFFFFFFF, 0x00000000     # the raw words that give u = 1.0 (the +0.5 ties to even at 2^24 - 1) and u = 2^-25


def u01(x):
    """the kernel's u01 in numpy float32: ((float)(x >> 8) + 0.5f) * 2^-24.  The sum rounds for x >> 8 >= 2^23 (ties to even:
    odd values lose the half upwards, even ones downwards), so the values lie in [2^-25, 1], both ends included"""
    top = (np.asarray(x, np.uint64) >> np.uint64(8)).astype(np.float32)
    return (top + F32(0.5)) * F32(1.0 / 16777216.0)


TWO_PI_F32 = F32(6.283185307179586)


def _draw_words(index, reps, seed):
    """raw words [len(index), reps, 4] of counter (Gaussian index, replica, 0, 0), key = the two halves of ``seed``"""
    seed = int(seed) & (2 ** 64 - 1)
    i = np.asarray(index, np.uint64).reshape(-1, 1)
    r = np.arange(reps, dtype=np.uint64).reshape(1, -1)
    w = philox4x32_10_np(i, r, 0, 0, seed & _MASK, seed >> 32)
    return np.stack(w, -1)


def normals_ref(index, reps, seed):
    """(z [n, reps, 3] float64, r [n, reps, 3] float64): Box-Muller on the kernel's float32 uniforms and its float32 angle, the
    logarithm, root, cosine and sine in float64; the third normal is r1 cos(a1).  r is the radius each normal was formed with"""
    w = _draw_words(index, reps, seed)
    u = u01(w)
    a = (TWO_PI_F32 * u[..., [1, 3]]).astype(np.float32).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u[..., [0, 2]].astype(np.float64)))
    z = np.stack([r[..., 0] * np.cos(a[..., 0]), r[..., 0] * np.sin(a[..., 0]), r[..., 1] * np.cos(a[..., 1])], -1)
    return z, np.stack([r[..., 0], r[..., 0], r[..., 1]], -1)


def normals_f32(index, reps, seed):
    """the kernel's arithmetic in numpy float32"""
    u = u01(_draw_words(index, reps, seed))
    a = TWO_PI_F32 * u[..., [1, 3]]
    r = np.sqrt(F32(-2.0) * np.log(u[..., [0, 2]]))
    z = np.stack([r[..., 0] * np.cos(a[..., 0]), r[..., 0] * np.sin(a[..., 0]), r[..., 1] * np.cos(a[..., 1])], -1)
    assert z.dtype == np.float32
    return z


def normals_ratio(z, index, reps, seed):
    """worst |z - z_ref| / (K_BM * EPS32 * (1 + r)) of normals ``z`` [n, reps, 3]"""
    ref, r = normals_ref(index, reps, seed)
    return float((np.abs(np.asarray(z, np.float64) - ref) / (K_BM * EPS32 * (1.0 + r))).max()) if ref.size else 0.0


def to_rows(x):
    """[n, reps, ...] -> rows in the kernel's order rep * n + rank"""
    return np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape((-1,) + x.shape[2:])


# ---------------------------------------------------------------------------------------------------------------------
# children of a split
# ---------------------------------------------------------------------------------------------------------------------
def _rotation(q, dt):
    """(R [n,3,3], A [n,3,3]) in dtype ``dt``: R of q / |q|, A the sum of the magnitudes each entry is formed from"""
    q = np.asarray(q, dt)
    q = q / np.sqrt((q * q).sum(1, keepdims=True, dtype=dt))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = dt(1.0), dt(2.0)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y),
                  two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x),
                  two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)], -1).reshape(-1, 3, 3)
    a = np.abs
    A = np.stack([one + two * (y * y + z * z), two * (a(x * y) + a(r * z)), two * (a(x * z) + a(r * y)),
                  two * (a(x * y) + a(r * z)), one + two * (x * x + z * z), two * (a(y * z) + a(r * x)),
                  two * (a(x * z) + a(r * y)), two * (a(y * z) + a(r * x)), one + two * (x * x + y * y)], -1).reshape(-1, 3, 3)
    return R, A


def children_ref(position, scaling_raw, rotation_raw, mask, split_num, normals, radius=None):
    """float64 new_pos_scale (atlas_gs_optimizer.py:255-287) of the selected rows; ``normals`` [split_num * n_sel, 3] in row order
    rep * n_sel + rank.  -> dict(pos, scl [split_num * n_sel, 3], mag [..] the bar's magnitude of pos (entries by their
    operands, see K_POS), mag_value [..] the same with |R_kj| for the entries).  ``radius`` [split_num * n_sel, 3]: the normals
    are the restated generator's (``normals_ref``) while the code under test drew its own, each within K_BM EPS32 (1 + r) of
    them; that bar, carried through the sum, joins the position's: K_BM EPS32 sum_j A_kj exp(s_j) (1 + r_j)"""
    m = np.asarray(mask).astype(bool).reshape(-1)
    n = int(m.sum())
    p = np.asarray(position, np.float64)[m]
    s = np.asarray(scaling_raw, np.float64)[m]
    R, A = _rotation(np.asarray(rotation_raw)[m], np.float64)
    zn = np.asarray(normals, np.float64).reshape(split_num, n, 3)
    sm = zn * np.exp(s)[None]
    pos = np.einsum("nkj,rnj->rnk", R, sm) + p[None]
    mag = np.einsum("nkj,rnj->rnk", A, np.abs(sm)) + np.abs(p)[None]
    mag_value = np.einsum("nkj,rnj->rnk", np.abs(R), np.abs(sm)) + np.abs(p)[None]
    if radius is not None:
        drawn = (K_BM / K_POS) * np.exp(s)[None] * (1.0 + np.asarray(radius, np.float64).reshape(split_num, n, 3))
        mag = mag + np.einsum("nkj,rnj->rnk", A, drawn)
        mag_value = mag_value + np.einsum("nkj,rnj->rnk", np.abs(R), drawn)
    scl = np.broadcast_to((s - np.log(0.8 * split_num))[None], (split_num, n, 3))
    f = lambda x: np.ascontiguousarray(x).reshape(split_num * n, 3)
    return dict(pos=f(pos), scl=f(scl), mag=f(mag), mag_value=f(mag_value), n=n)


def children_f32(position, scaling_raw, rotation_raw, mask, split_num, normals):
    """the kernel's arithmetic in numpy float32 (no fused multiply-add) -> (new_pos, new_scaling)"""
    m = np.asarray(mask).astype(bool).reshape(-1)
    n = int(m.sum())
    p = np.asarray(position, np.float32)[m]
    s = np.exp(np.asarray(scaling_raw, np.float32)[m])
    R, _ = _rotation(np.asarray(rotation_raw, np.float32)[m], np.float32)
    zn = np.asarray(normals, np.float32).reshape(split_num, n, 3)
    sm = zn * s[None]
    pos = R[None, :, :, 0] * sm[:, :, None, 0] + R[None, :, :, 1] * sm[:, :, None, 1] + R[None, :, :, 2] * sm[:, :, None, 2] + p[None]
    scl = np.broadcast_to(np.log(s / (F32(0.8) * F32(split_num)))[None], (split_num, n, 3))
    assert pos.dtype == np.float32 and scl.dtype == np.float32
    return np.ascontiguousarray(pos).reshape(-1, 3), np.ascontiguousarray(scl).reshape(-1, 3)


def children_ratios(pos, scl, ref):
    """worst error / bar of children (pos, scl) against ``children_ref``'s result: (position, scale, position against the
    magnitude built from |R_kj|)"""
    if ref["n"] == 0:
        return 0.0, 0.0, 0.0
    dp = np.abs(np.asarray(pos, np.float64) - ref["pos"])
    ds = np.abs(np.asarray(scl, np.float64) - ref["scl"])
    with np.errstate(invalid="ignore", divide="ignore"):
        rp = np.where(dp == 0, 0.0, dp / (K_POS * EPS32 * ref["mag"]))
        rv = np.where(dp == 0, 0.0, dp / (K_POS * EPS32 * ref["mag_value"]))
    return float(rp.max()), float((ds / (K_SCL * EPS32 * (1.0 + np.abs(ref["scl"])))).max()), float(rv.max())


CHILD_N = (1, 257, 5000)
CHILD_SPLIT = (1, 2, 3, 5)
CHILD_MASKS = ("none", "all", "first", "last", "random")


def select_mask(kind, N, rng):
    m = np.zeros(N, bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "alternating":
        m[::2] = True
    elif kind == "blocks":                       # whole 256-row blocks selected next to empty ones
        m[:] = (np.arange(N) // 256) % 2 == 0
    elif kind == "random":
        m[:] = rng.random(N) < 0.41
    elif kind != "none":
        raise ValueError(kind)
    return m


def children_case(N, split_num, mask_kind, seed=0):
    """position [N,3], scaling_raw [N,3] (log-scales -12 .. +4, each axis on its own), rotation_raw [N,4] (any direction, norm 1e-6
    .. 1e6, never zero), mask, unit normals [split_num * n_sel, 3].  A third of the rows are far from the origin (|p| up to
    1e4) with scales of 1e-5: the offset is lost in the position's last bits, which the bar's |p_k| term covers"""
    rng = np.random.default_rng([seed, N, split_num, CHILD_MASKS.index(mask_kind)])
    pos = rng.normal(0, 2.0, size=(N, 3))
    scl = rng.uniform(-12.0, 4.0, size=(N, 3))
    far = rng.random(N) < 1.0 / 3.0
    pos[far] = rng.uniform(-1e4, 1e4, size=(int(far.sum()), 3))
    scl[far] = np.log(1e-5) + rng.normal(0, 0.1, size=(int(far.sum()), 3))
    q = rng.normal(size=(N, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * 10.0 ** rng.uniform(-6, 6, size=(N, 1))
    mask = select_mask(mask_kind, N, rng)
    n = int(mask.sum())
    zn = rng.normal(size=(split_num * n, 3))
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(id=f"N{N}.s{split_num}.{mask_kind}", position=f(pos), scaling_raw=f(scl), rotation_raw=f(q), mask=mask, normals=f(zn),
                split_num=split_num, n=n)


# ---------------------------------------------------------------------------------------------------------------------
# row movement in numpy (bit for bit)
# ---------------------------------------------------------------------------------------------------------------------
def truth(mask):
    """a mask as the kernels read it: any non-zero byte selects"""
    return np.asarray(mask).reshape(-1) != 0


def clone_np(params, moments, mask):
    m = truth(mask)
    p = {k: np.concatenate([v, v[m]]) for k, v in params.items()}
    mo = None if moments is None else {k: tuple(np.concatenate([x, np.zeros_like(x[m])]) for x in mv) for k, mv in moments.items()}
    return p, mo


def split_np(params, moments, mask, split_num, new_pos, new_scl, position="position", scaling="scaling"):
    """children appended (their positions and scales given), other attributes repeated in the order rep * n_sel + rank, zero
    moments, parents removed"""
    m = truth(mask)
    n = int(m.sum())
    valid = np.concatenate([~m, np.ones(split_num * n, bool)])
    p = {}
    for k, v in params.items():
        tail = new_pos if k == position else new_scl if k == scaling else np.tile(v[m], (split_num,) + (1,) * (v.ndim - 1))
        p[k] = np.concatenate([v, np.asarray(tail, v.dtype).reshape((split_num * n,) + v.shape[1:])])[valid]
    mo = None if moments is None else {k: tuple(np.concatenate([x, np.zeros((split_num * n,) + x.shape[1:], x.dtype)])[valid] for x in mv)
                                       for k, mv in moments.items()}
    return p, mo, valid


def morton_np(uv, W, H):
    """the Z-curve code of splat_morton_keys: 15 bits per axis of (u / W, v / H), outside positions clamped to the border"""
    def spread(v):
        v = v.astype(np.uint32)
        v = (v | (v << 8)) & 0x00FF00FF
        v = (v | (v << 4)) & 0x0F0F0F0F
        v = (v | (v << 2)) & 0x33333333
        return (v | (v << 1)) & 0x55555555
    uv = np.asarray(uv, np.float32)
    fx = np.clip(uv[:, 0] * np.float32(32768.0 / W), 0, 32767)
    fy = np.clip(uv[:, 1] * np.float32(32768.0 / H), 0, 32767)
    return spread(fx.astype(np.uint32)) | (spread(fy.astype(np.uint32)) << 1)
