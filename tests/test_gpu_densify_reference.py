"""The densification kernels (csrc/densify.hip through splatter_a_video_amd.densify) against the references of
tests/densify_ref.py: decisions against float64 with per-row margins, statistics against the float32 restatement bit for bit,
children against float64 per element, the generator against Philox-4x32-10 restated, row movement against numpy bit for bit.
Every test prints its worst error / bar; tools/densify_reference_report.py writes them to profiles/densify_reference_gpu.json."""
import numpy as np
import pytest
import torch

import densify_ref as dr
from splatter_a_video_amd import densify as D

pytestmark = pytest.mark.gpu
SEEDS = (0, 77, 2 ** 32 + 5, 2 ** 64 - 1)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _n(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_n(a) if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint8) if a.dtype == np.bool_ else a.view(np.int32) if a.dtype.itemsize == 4 else a


def _same(a, b, what=""):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), (what, int((a != b).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# decisions
# ---------------------------------------------------------------------------------------------------------------------
def run_masks(N, params):
    c = dr.mask_case(N, params)
    st = D.DensifyState(N, "cuda")
    st.pos_gradient_accum.copy_(_t(c["accum"]).view(N, 1)); st.denom.copy_(_t(c["denom"]).view(N, 1)); st.max_radii2D.copy_(_t(c["max_radii2D"]))
    got = [_n(m) for m in st.masks(_t(c["scaling_raw"]), _t(c["opacity_raw"]), *c["args"])]
    out = {}
    for k, a in zip(("clone", "split", "prune"), got):
        rows = dr.compared_rows(c, k)
        left_out = int((~rows).sum())
        out[k] = dict(left_out_share=left_out / N, differ_where_compared=float((a[rows] != c["ref"][k][rows]).sum()),
                      differ_where_left_out=float((a[~rows] != c["ref"][k][~rows]).sum()))
        print(f"{c['id']} {k}: left out {left_out} of {N} ({100.0 * left_out / N:.4f} %), selected {int(a.sum())}")
        assert left_out <= int(dr.EXCLUDE_CAP * N), (c["id"], k, left_out)
        bad = np.flatnonzero(rows & (a != c["ref"][k]))
        assert bad.size == 0, (c["id"], k, bad[:10], [dr.STRATA[s] for s in c["stratum"][bad[:10]]],
                               {q: d[bad[:10]] for q, d in c["ref"]["dist"].items()})
    return out


@pytest.mark.parametrize("params", sorted(dr.MASK_PARAMS))
@pytest.mark.parametrize("N", dr.MASK_N)
def test_masks_equal_the_float64_decisions_on_every_clear_and_tie_row(N, params):
    run_masks(N, params)


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
def _stats_equal(st, ref):
    _same(st.viewspace_grad, ref.viewspace_grad, "viewspace_grad")
    _same(st.visibility, ref.visibility, "visibility")
    _same(st.radii, ref.radii, "radii")
    _same(st.max_radii2D, ref.max_radii2D, "max_radii2D")
    _same(st.denom.view(-1), ref.denom, "denom")
    a, b = _n(st.pos_gradient_accum).reshape(-1).astype(np.float64), ref.accum64
    np.testing.assert_allclose(a, b, rtol=2e-6, atol=0)
    nz = b != 0
    return float((np.abs(a - b)[nz] / (2e-6 * np.abs(b[nz]))).max()) if nz.any() else 0.0


def run_stats(N):
    sent = dr.stats_sentinels(N, 3)
    ref = dr.StatsRef(N, sent)
    st = D.DensifyState(N, "cuda")
    st.max_radii2D.copy_(_t(sent["max_radii2D"])); st.pos_gradient_accum.copy_(_t(sent["pos_gradient_accum"]).view(N, 1))
    st.denom.copy_(_t(sent["denom"]).view(N, 1))
    worst = 0.0
    # a batch of three frames with taps (dL_duv and the (W / 2, H / 2) scale); radii <= 0 are not visible and raise no maximum
    st.begin_batch(); ref.begin_batch()
    for radius, tap in dr.stats_frames(N, 3, 0):
        st.accumulate_frame(_t(radius), _t(tap), scale=dr.STATS_SCALE)
        ref.accumulate_frame(radius, tap, dr.STATS_SCALE)
    _stats_equal(st, ref)
    st.update(); ref.update()
    worst = max(worst, _stats_equal(st, ref))
    unseen = ref.visibility == 0
    if unseen.any():                                   # update() left the rows it did not see as they were
        assert np.array_equal(_n(st.max_radii2D)[unseen], sent["max_radii2D"][unseen])
        assert np.array_equal(_n(st.denom).reshape(-1)[unseen], sent["denom"][unseen])
        assert np.array_equal(_n(st.pos_gradient_accum).reshape(-1)[unseen], sent["pos_gradient_accum"][unseen])
    # a batch without taps: viewspace_grad (here a pattern no kernel wrote) stays bit for bit
    st.begin_batch(); ref.begin_batch()
    rng = np.random.default_rng(N)
    pattern = (rng.normal(size=(N, 2)) * 10.0 ** rng.uniform(-6, 6, size=(N, 2))).astype(np.float32)
    st.viewspace_grad.copy_(_t(pattern)); ref.viewspace_grad[...] = pattern
    for radius, _ in dr.stats_frames(N, 2, 1, taps=False):
        st.accumulate_frame(_t(radius), None)
        ref.accumulate_frame(radius, None)
    _same(st.viewspace_grad, pattern, "viewspace_grad without a tap")
    st.update(); ref.update()
    _stats_equal(st, ref)
    # prune, then a further batch at the new N
    valid = np.random.default_rng(N + 1).random(N) < 0.6
    if N == 1:
        valid[:] = True
    st.prune_postprocess(_t(valid)); ref.prune_postprocess(valid)
    assert st.num_points == ref.N == int(valid.sum())
    _stats_equal(st, ref)
    M = ref.N
    st.begin_batch(); ref.begin_batch()
    for radius, tap in dr.stats_frames(M, 2, 2):
        st.accumulate_frame(_t(radius), _t(tap), scale=dr.STATS_SCALE)
        ref.accumulate_frame(radius, tap, dr.STATS_SCALE)
    st.update(); ref.update()
    _stats_equal(st, ref)
    print(f"statistics N{N}: pos_gradient_accum worst error / (rtol 2e-6) = {worst:.4g}")
    return worst


@pytest.mark.parametrize("N", [1, 255, 257, 70_001])
def test_statistics_sequences_equal_the_float32_restatement(N):
    run_stats(N)


# ---------------------------------------------------------------------------------------------------------------------
# children
# ---------------------------------------------------------------------------------------------------------------------
def run_children(N, split_num, kind):
    c = dr.children_case(N, split_num, kind)
    a = (c["position"], c["scaling_raw"], c["rotation_raw"], c["mask"], split_num, c["normals"])
    ref = dr.children_ref(*a)
    pos, scl, n = D.split_children(_t(c["position"]), _t(c["scaling_raw"]), _t(c["rotation_raw"]), _t(c["mask"]), split_num,
                                   unit_normals=_t(c["normals"]))
    assert n == c["n"] and tuple(pos.shape) == tuple(scl.shape) == (split_num * n, 3)
    rp, rs, rv = dr.children_ratios(_n(pos), _n(scl), ref)
    print(f"children {c['id']}: position {rp:.4g}, scale {rs:.4g} of the bar (position against |R_kj| magnitudes: {rv:.4g})")
    assert rp <= 1.0 and rs <= 1.0, (c["id"], rp, rs)
    return dict(pos=rp, scl=rs, pos_against_entry_values=rv)


@pytest.mark.parametrize("kind", dr.CHILD_MASKS)
@pytest.mark.parametrize("split_num", dr.CHILD_SPLIT)
@pytest.mark.parametrize("N", dr.CHILD_N)
def test_children_with_given_normals_meet_the_float64_bars(N, split_num, kind):
    run_children(N, split_num, kind)


def _draw(N, mask, split_num, seed):
    """the generator's normals for the selected rows: identity rotation, zero position, zero log-scale"""
    pos = torch.zeros(N, 3, device="cuda"); scl = torch.zeros(N, 3, device="cuda")
    rot = torch.zeros(N, 4, device="cuda"); rot[:, 0] = 1.0
    z, s, n = D.split_children(pos, scl, rot, _t(mask), split_num, seed=seed)
    assert n == int(mask.sum())
    return _n(z).reshape(split_num, n, 3).swapaxes(0, 1), _n(s)


def run_generator(seed, N=5000, split_num=3):
    full = np.ones(N, bool)
    z, s = _draw(N, full, split_num, seed)
    ratio = dr.normals_ratio(z, np.arange(N), split_num, seed)
    print(f"generator seed {seed}: worst error / Box-Muller bar = {ratio:.4g}")
    assert ratio <= 1.0, (seed, ratio)
    want = np.float64(-np.log(0.8 * split_num))
    assert (np.abs(s - want) <= dr.K_SCL * dr.EPS32 * (1.0 + abs(want))).all()
    return ratio, z


@pytest.mark.parametrize("seed", SEEDS)
def test_generated_normals_are_philox_box_muller(seed):
    _, z = run_generator(seed)
    if seed >> 32:                                     # the high seed word is part of the key
        low, _ = _draw(5000, np.ones(5000, bool), 3, seed & 0xFFFFFFFF)
        assert not np.array_equal(low, z)
        assert np.abs(low - z).max() > 1.0


def test_draws_of_a_gaussian_do_not_depend_on_the_selection():
    N, split_num, seed = 5000, 3, 77
    full, _ = _draw(N, np.ones(N, bool), split_num, seed)
    rng = np.random.default_rng(0)
    for kind in ("first", "last", "alternating", "blocks", "random"):
        m = dr.select_mask(kind, N, rng)
        sub, _ = _draw(N, m, split_num, seed)
        _same(sub, full[m], kind)
    two, _ = _draw(N, np.ones(N, bool), 2, seed)       # nor on the number of replicas
    _same(two, full[:, :2], "replicas")


# ---------------------------------------------------------------------------------------------------------------------
# row movement
# ---------------------------------------------------------------------------------------------------------------------
MOVE_N = (1, 255, 256, 257, 262_401)     # the last: 1026 scan blocks, past the single-workgroup scan's 1024-entry loop
MOVE_MASKS = ("none", "all", "first", "last", "alternating", "blocks", "random", "bytes")
INTERVALS = 5


def _move_mask(kind, N, rng):
    if kind == "bytes":                                # a uint8 mask holding 2 and 255 as "true"
        m = dr.select_mask("random", N, rng)
        return np.where(m, rng.choice(np.array([2, 255], np.uint8), size=N), 0).astype(np.uint8)
    return dr.select_mask(kind, N, rng)


def _patterns(rng, shape, dtype=np.float32):
    """any 32-bit pattern (NaN payloads and denormals among them): row movement must not touch a bit"""
    return rng.integers(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(np.int32).view(dtype)


def _cloud(N, rng, big):
    """row widths of 1, 3, 4 and 48 words and 12 * I, an int32 tensor and a non-contiguous input; position / scaling / rotation
    hold values the split kernel can compute with.  -> (params, moments, the same on the device, tensors for compact alone).  At
    the largest N the widest tensor goes through compact only and two tensors carry moments: the test stays quick"""
    p = {"position": rng.normal(size=(N, 3)).astype(np.float32), "scaling": rng.uniform(-6, 1, size=(N, 3)).astype(np.float32),
         "rotation": rng.normal(size=(N, 4)).astype(np.float32), "opacity": _patterns(rng, (N,)),
         "ids": _patterns(rng, (N, 2), np.int32)}
    extra = {}
    (extra if big else p)["shs"] = _patterns(rng, (N, 16, 3))
    if not big:
        p["pos_cubic_node"] = _patterns(rng, (N, 12 * INTERVALS))
    with_moments = ("position", "opacity") if big else [k for k, v in p.items() if v.dtype == np.float32]
    m = {k: (_patterns(rng, p[k].shape), _patterns(rng, p[k].shape)) for k in with_moments}
    dev_p = {k: _t(v) for k, v in p.items()}
    dev_p["position"] = _t(np.repeat(p["position"], 2, axis=1))[:, ::2]     # every second column of [N, 6]: a strided view
    assert not dev_p["position"].is_contiguous()
    dev_m = {k: (_t(a), _t(b)) for k, (a, b) in m.items()}
    return p, m, dev_p, dev_m, extra


def _state_equal(p, m, want_p, want_m, what):
    for k in want_p:
        _same(p[k], want_p[k], (what, k))
    for k in want_m:
        _same(m[k][0], want_m[k][0], (what, k, "exp_avg"))
        _same(m[k][1], want_m[k][1], (what, k, "exp_avg_sq"))


@pytest.mark.parametrize("N", MOVE_N)
def test_row_movement_equals_numpy_bit_for_bit(N):
    big = N > 100_000
    rng = np.random.default_rng(N)
    p, m, dev_p, dev_m, extra = _cloud(N, rng, big)
    every, dev_every = dict(p, **extra), dict(dev_p, **{k: _t(v) for k, v in extra.items()})
    for kind in MOVE_MASKS:
        mask = _move_mask(kind, N, rng)
        sel = dr.truth(mask)
        dmask = _t(mask)
        # compact / prune_points: rows kept in order
        out = D.compact(dmask, dev_every)
        for k in every:
            _same(out[k], every[k][sel], ("compact", kind, k))
        q, qm = D.prune_points(dev_p, dev_m, dmask)
        _state_equal(q, qm, {k: v[sel] for k, v in p.items()}, {k: (a[sel], b[sel]) for k, (a, b) in m.items()}, ("prune", kind))
        # clone: selected rows appended once, their moments zero
        q, qm, n = D.densify_clone(dev_p, dev_m, dmask)
        assert n == int(sel.sum())
        _state_equal(q, qm, *dr.clone_np(p, m, mask), ("clone", kind))
        # split: children appended in the order rep * n_sel + rank with zero moments, parents removed
        for split_num in (1, 3):
            new_pos, new_scl, n2 = D.split_children(dev_p["position"], dev_p["scaling"], dev_p["rotation"], dmask, split_num, seed=9)
            q, qm, valid, n3 = D.densify_split(dev_p, dev_m, dmask, split_num, seed=9)
            assert n2 == n3 == int(sel.sum())
            want_p, want_m, want_valid = dr.split_np(p, m, mask, split_num, _n(new_pos), _n(new_scl))
            _same(valid, want_valid, ("split valid", kind))
            _state_equal(q, qm, want_p, want_m, ("split", kind, split_num))


def test_row_movement_rejects_what_it_cannot_move():
    x = torch.zeros(4, 3, device="cuda", dtype=torch.float64)
    with pytest.raises(ValueError):
        D.compact(torch.ones(4, dtype=torch.bool, device="cuda"), {"x": x})
    with pytest.raises(ValueError):
        D.compact(torch.ones(5, dtype=torch.bool, device="cuda"), {"x": x.float()})


# ---------------------------------------------------------------------------------------------------------------------
def measure():
    """every ratio above, for tools/densify_reference_report.py"""
    out = {"masks": {}, "children": {}, "generator": {}, "statistics": {}}
    for N in dr.MASK_N:
        for params in sorted(dr.MASK_PARAMS):
            out["masks"][f"{params}.N{N}"] = run_masks(N, params)
    for N in (1, 255, 257, 70_001):
        out["statistics"][f"N{N}"] = run_stats(N)
    worst = dict(pos=0.0, scl=0.0, pos_against_entry_values=0.0)
    for N in dr.CHILD_N:
        for s in dr.CHILD_SPLIT:
            for kind in dr.CHILD_MASKS:
                r = run_children(N, s, kind)
                worst = {k: max(worst[k], r[k]) for k in worst}
    out["children"] = worst
    for seed in SEEDS:
        out["generator"][f"seed{seed}"] = run_generator(seed)[0]
    return out
