"""The Adam kernels (splat_adam_step / splat_adam_step_pattern behind optim.FlatAdam and optim.OwnerShardedAdam) against a float64
Adam (tests/adam_ref.py) on every cut of the flat buffer a schedule hands them: buffer lengths with every n % 4 (the kernel's
float4 body + scalar tail), group boundaries inside a float4, PatternLR periods that are not multiples of 4, 16 segments,
a buffer past one grid-stride trip; the blocks of ZeRO-1 (Zero1Shards, padded bucket) and of OwnerShards for every rank of a
world emulated in one process (OwnerShardedAdam.step makes no collective); TrainingStep(zero1=True) with a padded bucket; and the
bucket's zero fill (splat_fill_f32).  One GPU, no process group."""

import numpy as np
import pytest
import torch

from adam_ref import Adam64, f32, rate_map
from splatter_a_video_amd import _lib as L
from splatter_a_video_amd.optim import MAX_SEGMENTS, FlatAdam, OwnerShardedAdam, PatternLR
from splatter_a_video_amd.parallel import FlatGradBucket, OwnerShards, Zero1Shards

pytestmark = pytest.mark.gpu

EPS = 1e-15
REF_BETAS = (f32(0.9), f32(0.999))          # FlatAdam's default betas as the kernel receives them
SHS = PatternLR(1.25e-4, head_lr=2.5e-3, period=48, head=3)     # the reference's SH groups
P7 = PatternLR(1e-3, head_lr=1e-2, period=7, head=2)


def _rates(slices, lrs, total):
    """the float64 reference's per-element rate, each rate as the float32 the ABI carries"""
    return rate_map(slices, lrs, total).astype(np.float32).astype(np.float64)


def _grad(rng, n, step):
    return (rng.standard_normal(n) * (0.1 + step % 5)).astype(np.float32)


def _scale(step):
    return 0.5 if step % 3 == 1 else (0.25 if step % 7 == 6 else 1.0)


def _bucket(sizes, rng, **kw):
    init = {k: rng.standard_normal(s).astype(np.float32) for k, s in sizes.items()}
    return FlatGradBucket({k: torch.from_numpy(v).cuda() for k, v in init.items()}, **kw)


# ------------------------------------------------------------------------------------------------ a. FlatAdam
def _layout(n):
    """groups of a flat buffer of n floats: boundaries inside a float4, a PatternLR of period 7 next to the reference's (48, 3),
    both starting at offsets that are no multiple of their period, two plain groups of equal rate that share a segment"""
    small = {1: {"a": 1}, 2: {"a": 1, "p7": 1}, 3: {"a": 1, "p7": 2}, 5: {"a": 1, "p7": 3, "b": 1}}
    if n in small:
        return small[n]
    return {"a": 149, "p7": 7010, "shs": 48000, "b": 3, "c": n - 149 - 7010 - 48000 - 3}


LR0 = {"a": 1e-2, "p7": P7, "shs": SHS, "b": 1e-3, "c": 1e-3}
K = 25000


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4 * K + 1, 4 * K + 2, 4 * K + 3])
def test_flat_adam_against_float64_adam(n):
    """30 steps: learning-rate changes that split and re-merge segments and swap a pattern for a plain rate, an all-zero gradient
    step, grad_scale 0.5 / 0.25; parameters and both moments within float32 rounding of float64 Adam after every step"""
    rng = np.random.default_rng(n)
    sizes = _layout(n)
    assert sum(sizes.values()) == n
    bucket = _bucket(sizes, rng)
    lr = {k: LR0[k] for k in sizes}
    opt = FlatAdam(bucket, lr, eps=EPS)
    ref = Adam64(bucket.flat_param.cpu().numpy(), betas=REF_BETAS, eps=f32(EPS))
    for step in range(30):
        if step == 8 and "b" in lr:
            nseg = opt.nseg
            lr["b"] = 5e-2                                             # b splits off c
            opt.set_lr({"b": 5e-2})
            assert opt.nseg == nseg + ("c" in lr)
        if step == 16 and "b" in lr:
            lr["b"] = 1e-3                                             # and merges again
            opt.set_lr({"b": 1e-3})
        if step == 20 and "p7" in lr:
            lr["p7"] = 2e-3                                            # pattern -> plain rate
            opt.set_lr({"p7": 2e-3})
        if step == 24 and "shs" in lr:
            lr["shs"] = PatternLR(5e-4, head_lr=1e-2, period=48, head=3)
            opt.set_lr({"shs": lr["shs"]})
        g = np.zeros(n, np.float32) if step == 5 else _grad(rng, n, step)
        bucket.flat_grad.copy_(torch.from_numpy(g))
        opt.step(grad_scale=_scale(step))
        ref.step(g, _rates(bucket.slices, lr, n), grad_scale=f32(_scale(step)))
        ref.check(bucket.flat_param.cpu().numpy(), opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy(), what=f"n={n} step {step}")


def test_flat_adam_with_16_segments_and_the_17th_refused():
    """MAX_SEGMENTS (= the kernel's SPLAT_ADAM_MAX_SEGMENTS) segments are stepped right; a 17th is a ValueError on the host,
    before anything is launched"""
    rng = np.random.default_rng(16)
    sizes = {f"g{i}": 5 + 3 * i for i in range(MAX_SEGMENTS + 1)}
    lr = {k: (P7 if i % 5 == 2 else 1e-3 * (1 + i % 2)) for i, k in enumerate(sizes)}
    lr["g16"] = lr["g15"]                                              # 17 groups, the last two share a segment
    bucket = _bucket(sizes, rng)
    n = bucket.flat_param.numel()
    opt = FlatAdam(bucket, lr, eps=EPS)
    assert opt.nseg == MAX_SEGMENTS
    ref = Adam64(bucket.flat_param.cpu().numpy(), betas=REF_BETAS, eps=f32(EPS))
    for step in range(5):
        g = _grad(rng, n, step)
        bucket.flat_grad.copy_(torch.from_numpy(g))
        opt.step(grad_scale=_scale(step))
        ref.step(g, _rates(bucket.slices, lr, n), grad_scale=f32(_scale(step)))
    ref.check(bucket.flat_param.cpu().numpy(), opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy(), what="16 segments")
    torch.cuda.synchronize()
    before = bucket.flat_param.clone()
    with pytest.raises(ValueError):
        opt.set_lr({"g16": 7e-3})                                      # g16 splits off g15: a 17th segment
    with pytest.raises(ValueError):
        FlatAdam(bucket, dict(lr, g16=7e-3))
    torch.cuda.synchronize()
    assert torch.equal(bucket.flat_param, before)


def test_flat_adam_past_one_grid_stride_trip():
    """n > 8192 blocks x 256 threads x 4 floats with n % 4 = 3: the grid-stride loop's second trip and the scalar tail"""
    n = 9_000_003
    assert n > 8192 * 256 * 4 and n % 4 == 3
    rng = np.random.default_rng(9)
    sizes = {"a": 4001, "shs": 48 * 170000, "p7": 7 * 31000 + 2}
    sizes["c"] = n - sum(sizes.values())
    lr = {"a": 1e-2, "shs": SHS, "p7": P7, "c": 3e-3}
    bucket = _bucket(sizes, rng)
    opt = FlatAdam(bucket, lr, eps=EPS)
    ref = Adam64(bucket.flat_param.cpu().numpy(), betas=REF_BETAS, eps=f32(EPS))
    rates = _rates(bucket.slices, lr, n)
    for step in range(3):
        g = _grad(rng, n, step)
        bucket.flat_grad.copy_(torch.from_numpy(g))
        opt.step(grad_scale=_scale(step))
        ref.step(g, rates, grad_scale=f32(_scale(step)))
    ref.check(bucket.flat_param.cpu().numpy(), opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy(), what="9M floats")


# ------------------------------------------------------------------------------------------------ b. every rank in one process
N_Z = 107
ZERO1_SIZES = {"cubic": (2, N_Z, 4, 3), "rotation": (N_Z, 4), "opacity": (N_Z, 1), "shs": (N_Z, 16, 3), "p7": (28 * N_Z + 1,),
               "attrs": (N_Z, 1)}
ZERO1_LR = {"cubic": 2e-3, "rotation": 5e-3, "opacity": 5e-2, "shs": SHS, "p7": P7, "attrs": 2e-2}
TINY_SIZES = {"a": (5,), "p7": (8,)}                  # 13 floats at world 8: blocks of 4, ranks 4..7 hold padding only
TINY_LR = {"a": 1e-2, "p7": P7}


def _pattern_cuts(slices, lr, cuts):
    """{(group, 'mid' | 'past')}: cuts that land inside a PatternLR period's head (phase 0 < ph < head) or behind it"""
    seen = set()
    for c in cuts:
        for k, (a, b) in slices.items():
            r = lr[k]
            if isinstance(r, PatternLR) and a < c < b and (c - a) % r.period:
                seen.add((k, "mid" if (c - a) % r.period < r.head else "past"))
    return seen


def _emulate_ranks(sizes, lr, world, make_shards, pad_to, steps=4):
    """every rank of `world` on a replica of the bucket, each stepping ITS cut with OwnerShardedAdam from the same gradient; the
    union of the owned blocks (+ the replicated slice) against FlatAdam on an unpadded twin (bit for bit) and float64 Adam"""
    rng = np.random.default_rng(world)
    init = {k: rng.standard_normal(s).astype(np.float32) for k, s in sizes.items()}
    mk = lambda **kw: FlatGradBucket({k: torch.from_numpy(v).cuda() for k, v in init.items()}, **kw)
    twin = mk()
    real = twin.flat_param.numel()
    flat = FlatAdam(twin, lr, eps=EPS)
    ranks = []
    for r in range(world):
        b = mk(pad_to=pad_to)
        ranks.append((b, OwnerShardedAdam(b, make_shards(b, r), lr, eps=EPS)))
    total = ranks[0][0].flat_param.numel()
    assert total > real, "the case must pad"
    start = ranks[0][0].flat_param.clone()
    ref = Adam64(twin.flat_param.cpu().numpy(), betas=REF_BETAS, eps=f32(EPS))
    rates = _rates(twin.slices, lr, real)
    for step in range(steps):
        g = _grad(rng, real, step)
        gt = torch.from_numpy(g).cuda()
        twin.flat_grad.copy_(gt)
        for b, o in ranks:
            b.zero_grad()
            b.flat_grad[:real].copy_(gt)                 # the padding's gradient is 0, as after the reduce-scatter
            o.step(grad_scale=_scale(step))
        flat.step(grad_scale=_scale(step))
        ref.step(g, rates, grad_scale=f32(_scale(step)))
    union = [torch.full((total,), float("nan"), device="cuda") for _ in range(3)]
    for r, (b, o) in enumerate(ranks):
        sh = o.shards
        lo, hi = sh.own
        union[0][lo:hi], union[1][lo:hi], union[2][lo:hi] = b.flat_param[lo:hi], o.m_own, o.v_own
        # this replica's other owned blocks are untouched (they come from their owners by the all-gather)
        assert torch.equal(b.flat_param[sh.a:lo], start[sh.a:lo]) and torch.equal(b.flat_param[hi:sh.b], start[hi:sh.b]), r
        pad = max(real - lo, 0)
        assert o.m_own[pad:].count_nonzero() == 0 and o.v_own[pad:].count_nonzero() == 0, r
        if sh.b < sh.total:                              # the replicated slice: every rank steps it alike
            assert torch.equal(b.flat_param[sh.b:], ranks[0][0].flat_param[sh.b:]), r
            union[0][sh.b:], union[1][sh.b:], union[2][sh.b:] = b.flat_param[sh.b:], o.m_rep, o.v_rep
            rp = max(real - sh.b, 0)
            assert o.m_rep[rp:].count_nonzero() == 0 and o.v_rep[rp:].count_nonzero() == 0, r
    p, m, v = union
    assert torch.equal(p[:real], twin.flat_param), "parameters: not FlatAdam's bits"
    assert torch.equal(m[:real], flat.exp_avg) and torch.equal(v[:real], flat.exp_avg_sq), "moments: not FlatAdam's bits"
    assert p[real:].count_nonzero() == 0 and m[real:].count_nonzero() == 0 and v[real:].count_nonzero() == 0, "padding moved"
    ref.check(p[:real].cpu().numpy(), m[:real].cpu().numpy(), v[:real].cpu().numpy(), what=f"world {world}")


def test_zero1_blocks_of_every_rank_against_flat_adam_and_float64():
    """Zero1Shards on a FlatGradBucket(pad_to=4 * world) whose real length is no multiple of 4 * world: the last rank's block
    ends in padding; in the tiny world-8 case several blocks are padding only"""
    real = sum(int(np.prod(s)) for s in ZERO1_SIZES.values())
    slices, o = {}, 0
    for k, s in ZERO1_SIZES.items():
        slices[k] = (o, o + int(np.prod(s)))
        o += int(np.prod(s))
    seen = set()
    for world in (1, 2, 3, 4, 8):
        assert real % (4 * world)
        per = -(-real // (4 * world)) * 4
        seen |= _pattern_cuts(slices, ZERO1_LR, [r * per for r in range(1, world)])
        _emulate_ranks(ZERO1_SIZES, ZERO1_LR, world, lambda b, r, w=world: Zero1Shards(b, w, r), 4 * world)
    # the blocks start inside a pattern's head (what is left of it keeps the head rate) and behind it, in both periods
    assert {("shs", "mid"), ("shs", "past"), ("p7", "mid"), ("p7", "past")} <= seen, seen
    _emulate_ranks(TINY_SIZES, TINY_LR, 8, lambda b, r: Zero1Shards(b, 8, r), 32)


@pytest.mark.parametrize("world", [2, 3, 5])
def test_owner_shards_of_every_rank_against_flat_adam_and_float64(world):
    """OwnerShards of a 7-unit table (no multiple of world) + a replicated slice with both PatternLR groups and padding behind it
    (pad_to=4 on an odd length)"""
    N = 41
    sizes = {"cubic": (7, N, 4, 3), "rotation": (N, 4), "opacity": (N, 1), "shs": (N, 16, 3), "p7": (7 * N + 4,), "attrs": (N, 1)}
    _emulate_ranks(sizes, ZERO1_LR, world, lambda b, r: OwnerShards(b, "cubic", world, r), 4)


# ------------------------------------------------------------------------------------------------ c. TrainingStep(zero1=True)
def test_training_step_zero1_on_a_padded_bucket_matches_the_dense_step():
    """world 1, A = 1 (12 I + 57 floats per Gaussian) and an odd Gaussian count: the ZeRO-1 bucket is padded to a multiple of 4.
    Steps, a densification rebuild, more steps: the dense TrainingStep's parameters (to the ARAP scatter's float atomics), the
    padding tail 0 throughout"""
    from test_gpu_train_step import _perturbed, _t

    from splatter_a_video_amd import train_step as TS
    from splatter_a_video_amd.dynamics import FrameClock
    from splatter_a_video_amd.synth import make_scene
    Nn, Ww, Hh, T, F = 2501, 128, 96, 20, 3
    sc = make_scene(Nn, Ww, Hh, F=T, seed=11, sigma_px=3.0)
    clock = FrameClock(T)
    truth = TS.synthetic_video_params(sc, clock, "cuda", attrs=1, seed=12, cubic_sigma=0.01)
    extr = _t(sc.extr)
    lr = dict(TS.REFERENCE_LR, pos_cubic_node=2e-3, shs=2e-2, attrs=2e-2, scaling=1e-2, rotation=5e-3)
    cfg = TS.DensifyConfig(interval=2, start_iter=0, grad_threshold=1e-6, cameras_extent=60.0, min_opacity=0.005, seed=1)
    t1, t2 = [0, 7, 13], [4, 2, 19]
    gt = TS.render_ground_truth(truth, clock, Ww, Hh, extr, t1, t2)
    out = {}
    for zero1 in (False, True):
        st = TS.TrainingStep(_perturbed(truth, 1), clock, Ww, Hh, F, extr, lr=lr, K=8, arap_samples=128, sample_seed=3,
                             densify=cfg, zero1=zero1)
        snaps = []
        for phase in range(2):
            for _ in range(3):
                st.step(t1, t2, gt)
            torch.cuda.synchronize()
            n = sum(v.numel() for v in st.p.values())
            snaps.append((st.N, st.bucket.flat_param[:n].clone()))
            if zero1:
                assert st.bucket.flat_param.numel() % 4 == 0
                assert st.bucket.flat_param[n:].count_nonzero() == 0
                assert st.opt.m_own[n:].count_nonzero() == 0 and st.opt.v_own[n:].count_nonzero() == 0
                if phase == 0:
                    assert st.bucket.flat_param.numel() > n, "the case must pad"
            if phase == 0:
                st.densify()
        assert torch.isfinite(st.bucket.flat_param).all()
        out[zero1] = snaps
    for (n_d, p_d), (n_z, p_z) in zip(out[False], out[True]):
        assert n_d == n_z
        torch.testing.assert_close(p_z, p_d, rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------ d. splat_fill_f32
FILL_N = list(range(10)) + [4001, 4002, 4003, 4096 * 256 * 4 + 43]


@pytest.mark.parametrize("n", FILL_N)
def test_fill_at_every_alignment_leaves_its_neighbours_alone(n):
    """n floats at 0..3 floats past a 16-byte boundary: the kernel's head up to alignment, float4 body (past one grid-stride trip
    at the largest n), scalar tail -- equal to torch's fill_, canaries on both sides untouched"""
    for off in range(4):
        buf = torch.full((off + n + 8,), -7.0, device="cuda")
        assert buf.data_ptr() % 16 == 0
        want = buf.clone()
        want[off:off + n].fill_(1.25)
        L.check(L.lib().splat_fill_f32(L.ptr(buf[off:]), n, 1.25, L.stream()))
        torch.cuda.synchronize()
        assert torch.equal(buf, want), (n, off)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 9, 4001, 4002, 4003])
def test_zero_grad_fills_the_active_buffer_only(n):
    """FlatGradBucket.zero_grad (splat_fill_f32 over the active gradient buffer): all of it 0, the other buffer untouched"""
    b = FlatGradBucket({"a": torch.ones(n, device="cuda")}, buffers=2)
    b.flat_grads[0].fill_(3.0)
    b.flat_grads[1].fill_(5.0)
    b.activate(1)
    b.zero_grad()
    torch.cuda.synchronize()
    assert b.flat_grads[1].count_nonzero() == 0 and torch.equal(b.flat_grads[0], torch.full((n,), 3.0, device="cuda"))
    assert b.params["a"].grad.data_ptr() == b.flat_grads[1].data_ptr()
