"""TrainingStep.densify() against a numpy restatement of the surgery, row by row: parameters, frozen tables and both Adam
moments are gathered out of the flat bucket (the spline table and its moments through the segment-major / Gaussian-major
conversions), cloned, split, pruned on fresh statistics, put in Morton order and laid into a new bucket.  Survivors must be
the bits they were, clones their source's bits, children their parent's other attributes, every new row's moments zero; the
children's positions and scales meet the bars of tests/densify_ref.py against the Philox restatement's normals.  The clone
and split DECISIONS are the device's own (tests/test_gpu_densify_reference.py judges them)."""
import numpy as np
import pytest
import torch

import densify_ref as dr
from splatter_a_video_amd import train_step as TS
from splatter_a_video_amd.dynamics import GAUSSIAN_MAJOR, frame_table, positions_batch_forward
from splatter_a_video_amd.gs.point_ops import project_point_ortho
from test_gpu_train_step import _clip, _perturbed, _t

pytestmark = pytest.mark.gpu
MODES = {"flat": {}, "owner_sharded": dict(owner_sharded=True), "zero1": dict(zero1=True)}     # the last two: one process owns all


def _np(t):
    return t.detach().cpu().numpy().copy()


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), (what, int((a.view(np.int32) != b.view(np.int32)).sum()))


def run(mode):
    N, W, H, T, F = 3000, 128, 96, 20, 4
    sc, clock, truth = _clip(N, W, H, T, seed=11)
    extr = _t(sc.extr)
    st = TS.TrainingStep(_perturbed(truth, 6), clock, W, H, F, extr, K=8, arap_samples=128, **MODES[mode])
    t1, t2 = [0, 3, 7, 12], [5, 1, 19, 2]
    gt = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
    for _ in range(3):
        st.step(t1, t2, gt)
    st.set_lr({"pos_cubic_node": 1.5e-5})
    # ---- snapshot
    p0, m0 = st._gather()
    p0 = {k: _np(v) for k, v in p0.items()}
    m0 = {k: (_np(a), _np(b)) for k, (a, b) in m0.items()}
    assert sorted(p0) == sorted(TS.TRAINABLE + TS.FROZEN) and sorted(m0) == sorted(TS.TRAINABLE)
    assert all(float(np.abs(a).max()) > 0 and float(b.max()) > 0 for a, b in m0.values())      # the moments are populated
    acc, den, mr = _np(st.dstate.pos_gradient_accum).reshape(-1), _np(st.dstate.denom).reshape(-1), _np(st.dstate.max_radii2D)
    t0, lr0, lr_own0, hist0, it0 = st.opt.t, dict(st.opt.lr), dict(st.lr), list(st.history), st.iteration
    assert t0 == 3 and it0 == 3
    # ---- a configuration that clones, splits and prunes a good share of THIS state (thresholds at its quantiles)
    seen = den > 0
    g = acc[seen].astype(np.float64) / den[seen]
    smax = np.exp(p0["scaling"].astype(np.float64).max(1))
    opac = 1.0 / (1.0 + np.exp(-p0["opacity"].astype(np.float64).reshape(-1)))
    extent = 10.0 * float(np.quantile(smax, 0.95))                     # 0.1 * extent: the largest 5 % are pruned by world size
    cfg = TS.DensifyConfig(grad_threshold=float(np.median(g)), percent_dense=float(np.median(smax)) / extent, cameras_extent=extent,
                           min_opacity=float(np.quantile(opac, 0.05)), split_num=2, size_threshold=20.0, seed=31)
    st.cfg = cfg
    args = (cfg.grad_threshold, cfg.percent_dense, cfg.cameras_extent, cfg.min_opacity, cfg.size_threshold)
    th = dr.thresholds(*args)
    clone, split, _ = st.dstate.masks(st.p["scaling"].detach(), st.p["opacity"].detach(), *args)
    clone, split = _np(clone), _np(split)

    st.densify()

    # ---- the surgery in numpy, from the snapshot; origin of every row: (kind 0 original / 1 clone / 2 child, source row, child row)
    tag = lambda n, kind: np.stack([np.full(n, kind), np.arange(n), np.full(n, -1)], 1).astype(np.int32)
    p = dict(p0, _tag=tag(N, 0))
    p, m = dr.clone_np(p, m0, clone)
    n_clone = int(clone.sum())
    p["_tag"][N:, 0] = 1
    split1 = np.concatenate([split, np.zeros(n_clone, bool)])          # the clones carry no gradient: never split
    n_split = int(split1.sum())
    z, r = dr.normals_ref(np.flatnonzero(split1), cfg.split_num, cfg.seed + it0)
    kids = dr.children_ref(p["position"], p["scaling"], p["rotation"], split1, cfg.split_num, dr.to_rows(z), radius=dr.to_rows(r))
    p, m, valid = dr.split_np(p, m, split1, cfg.split_num, kids["pos"].astype(np.float32), kids["scl"].astype(np.float32))
    n_kids = cfg.split_num * n_split
    p["_tag"][len(valid[valid]) - n_kids:, 0] = 2
    p["_tag"][len(valid[valid]) - n_kids:, 2] = np.arange(n_kids)
    M = p["position"].shape[0]
    zero = np.zeros(M, np.float32)
    fresh = dr.masks_ref(zero, zero, zero, p["scaling"], p["opacity"], th)          # prune after the statistics were reset
    assert fresh["clear"]["prune"].all(), "a row of this fixture sits on a prune threshold: pick another seed"
    keep = ~fresh["prune"]
    n_prune = int(fresh["prune"].sum())
    print(f"{mode}: N {N} -> {st.N}: cloned {n_clone}, split {n_split}, pruned {n_prune}")
    assert n_clone >= 50 and n_split >= 50 and n_prune >= 50
    assert st.last_change == dict(cloned=n_clone, split=n_split, pruned=n_prune, N=int(keep.sum()))
    p = {k: v[keep] for k, v in p.items()}
    m = {k: (a[keep], b[keep]) for k, (a, b) in m.items()}
    N2 = st.N
    assert N2 == int(keep.sum()) == N + n_clone + (cfg.split_num - 1) * n_split - n_prune

    # ---- the recorded order: the stable argsort of the Morton code of the screen positions it was computed from
    perm = _np(st.last_order)
    assert perm.shape == (N2,) and np.array_equal(np.sort(perm), np.arange(N2))
    pn, mn = st._gather()
    tab0 = frame_table(clock, [0], st.dev)
    pos0 = positions_batch_forward(tab0, pn["position"].contiguous(), pn["pos_cubic_node"].reshape(N2, -1).contiguous(), clock.interval_num,
                                   GAUSSIAN_MAJOR)[0]
    with torch.no_grad():
        uv_new, _ = project_point_ortho(pos0, extr, W, H, nearest=0.01)
    uv = np.empty((N2, 2), np.float32)
    uv[perm] = _np(uv_new)                                             # row i now was row perm[i] when the order was taken
    assert np.array_equal(np.argsort(dr.morton_np(uv, W, H), kind="stable"), perm)

    # ---- every row against the restatement
    pn = {k: _np(v) for k, v in pn.items()}
    mn = {k: (_np(a), _np(b)) for k, (a, b) in mn.items()}
    want_p = {k: v[perm] for k, v in p.items()}
    want_m = {k: (a[perm], b[perm]) for k, (a, b) in m.items()}
    kind, src, kid = want_p["_tag"][:, 0], want_p["_tag"][:, 1], want_p["_tag"][:, 2]
    old, new, child = kind == 0, kind != 0, kind == 2
    assert old.sum() > 1000 and (kind == 1).sum() >= 25 and child.sum() >= 50
    for k in TS.TRAINABLE + TS.FROZEN:
        rows = ~child if k in ("position", "scaling") else np.ones(N2, bool)
        _same(pn[k][rows], want_p[k][rows], k)
        _same(pn[k][old], p0[k][src[old]], (k, "survivors are the snapshot's bits"))
        if k not in ("position", "scaling"):
            parent = src[new]                                          # a clone's source, a child's parent: rows of the snapshot
            _same(pn[k][new], p0[k][parent], (k, "new rows carry their source's bits"))
    for k in TS.TRAINABLE:
        for j, name in enumerate(("exp_avg", "exp_avg_sq")):
            _same(mn[k][j], want_m[k][j], (k, name))
            _same(mn[k][j][old], m0[k][j][src[old]], (k, name, "survivors keep their moments"))
            assert not mn[k][j][new].any(), (k, name, "new rows start with zero moments")
    _same(pn["position"][kind == 1], p0["position"][src[kind == 1]], "a clone's position")
    _same(pn["scaling"][kind == 1], p0["scaling"][src[kind == 1]], "a clone's scale")
    ref = {k: kids[k][kid[child]] for k in ("pos", "scl", "mag", "mag_value")}
    ref["n"] = int(child.sum())
    rp, rs, _ = dr.children_ratios(pn["position"][child], pn["scaling"][child], ref)
    print(f"{mode}: children of the step: position {rp:.4g}, scale {rs:.4g} of the bar")
    assert rp <= 1.0 and rs <= 1.0, (rp, rs)

    # ---- the optimiser and the statistics continue
    assert st.opt.t == t0 and st.opt.lr == lr0 and st.lr == lr_own0 and st.opt.lr["pos_cubic_node"] == 1.5e-5
    assert st.history == hist0 + [N2] and st.iteration == it0
    d = st.dstate
    assert d.num_points == N2
    for t, shape in ((d.max_radii2D, (N2,)), (d.pos_gradient_accum, (N2, 1)), (d.denom, (N2, 1)), (d.viewspace_grad, (N2, 2)),
                     (d.visibility, (N2,)), (d.radii, (N2,))):
        assert tuple(t.shape) == shape and not bool(t.any())
    st.fb.check()
    st.step(t1, t2, gt)
    assert torch.isfinite(st.bucket.flat_param).all() and torch.isfinite(st.bucket.flat_grad).all() and np.isfinite(st.loss())
    assert st.opt.t == t0 + 1
    return dict(pos=rp, scl=rs)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_densify_moves_every_row_with_its_moments_and_tables(mode):
    run(mode)
