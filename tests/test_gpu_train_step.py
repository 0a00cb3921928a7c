"""The reference's training step composed from the native pieces (splatter_a_video_amd/train_step.py; reference:
src/trainer_fragGS.py:470-790): the new operators against the reference-made fixture / the CPU oracle, the training frame WITH
its track_gs leg against the oracle chain, and the whole step -- convergence on a synthetic clip with a changing Gaussian
count."""
import os

import numpy as np
import pytest
import torch

import oracle_chain as oc
from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import train_step as TS
from splatter_a_video_amd.arap import cal_arap_error, pair_arap, pair_connectivity
from splatter_a_video_amd.dynamics import (GAUSSIAN_MAJOR, SEGMENT_MAJOR, FrameClock, evaluate, frame_table, positions_batch,
                                           to_gaussian_major, to_segment_major)
from splatter_a_video_amd.frames import FrameBatch
from splatter_a_video_amd.knn import knn_brute_batch, knn_points
from splatter_a_video_amd.synth import make_scene
from test_gpu_parity import GRAD_RTOL, IMG_ATOL, IMG_RTOL, assert_grad

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _t(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda", requires_grad=grad)


# ---------------------------------------------------------------------------------------------------------------------
def test_positions_batch_against_the_reference_fixture():
    """positions of ALL frame times in one launch each way = get_position(t) of the reference per frame (golden vectors made by
    DynamicGaussianWithBasePointCloud.get_position + autograd, tests/golden/make_golden_dynamic.py), both spline layouts"""
    g = dict(np.load(os.path.join(GOLD, "dynamic_400x50.npz")))
    clock = FrameClock(int(g["T"]), g["intervals"], int(g["start_frame_id"]), int(g["time_len"]))
    I = clock.interval_num
    times = [int(t) for t in g["times"]]
    want_d_cubic = sum(g[f"t{t}_d_cubic"].astype(np.float64) for t in times)
    want_d_pos = sum(g[f"t{t}_d_position"].astype(np.float64) for t in times)
    gpos = torch.stack([_t(g[f"t{t}_g_pos"]) for t in times])
    for layout in (GAUSSIAN_MAJOR, SEGMENT_MAJOR):
        pos = _t(g["position"], True)
        cub = _t(g["pos_cubic_node"])
        cub = (to_segment_major(cub, I) if layout == SEGMENT_MAJOR else cub).requires_grad_(True)
        out = positions_batch(clock, times, pos, cub, cubic_layout=layout)
        for f, t in enumerate(times):
            np.testing.assert_allclose(out[f].detach().cpu().numpy(), g[f"t{t}_pos"], rtol=3e-6, atol=3e-6)
        out.backward(gpos)
        dc = to_gaussian_major(cub.grad) if layout == SEGMENT_MAJOR else cub.grad
        np.testing.assert_allclose(dc.cpu().numpy(), want_d_cubic, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(pos.grad.cpu().numpy(), want_d_pos, rtol=1e-5, atol=1e-6)
    # an unsorted table with repeated segments (the random pair frames of a batch) = the sum of single-frame evaluations
    times2 = [44, 1, 45, 0, 44, 25]
    pos, cub = _t(g["position"], True), _t(g["pos_cubic_node"], True)
    gp = torch.randn(len(times2), pos.shape[0], 3, device="cuda")
    positions_batch(clock, times2, pos, cub).backward(gp)
    p2, c2 = _t(g["position"], True), _t(g["pos_cubic_node"], True)
    for f, t in enumerate(times2):
        evaluate(clock, t, position=p2, pos_cubic_node=c2)[0].backward(gp[f])
    assert torch.allclose(cub.grad, c2.grad, rtol=1e-5, atol=1e-6) and torch.allclose(pos.grad, p2.grad, rtol=1e-5, atol=1e-6)


def test_brute_force_knn_is_the_grid_knn_of_the_sampled_vertices():
    """K + 1 nearest neighbours of a few query vertices per point set, brute force = the rows of the exact grid search over the
    whole set (knn_points, checked against the oracle in test_gpu_knn.py); strided batches; a duplicated point (tie)"""
    rng = np.random.default_rng(3)
    B, N, S, K = 3, 20000, 300, 6
    pts = rng.uniform(-1, 1, size=(B, 2, N, 3)).astype(np.float32)
    pts[1, 0, 77] = pts[1, 0, 5]                                   # exact tie: the smaller index first
    buf = _t(pts)
    view = buf[:, 0]                                               # batch stride 2 N 3: read in place
    q = torch.from_numpy(np.stack([rng.choice(N, S, replace=False) for _ in range(B)])).cuda()
    q[1, 0] = 77
    d, i = knn_brute_batch(view, q, K)
    for b in range(B):
        ref = knn_points(view[b].contiguous()[None], view[b].contiguous()[None], K=K)
        assert torch.equal(i[b].long(), ref.idx[0][q[b]])
        assert torch.allclose(d[b], ref.dists[0][q[b]], rtol=1e-6, atol=1e-9)
    assert int(i[1, 0, 0]) == 5 and int(i[1, 0, 1]) == 77 and float(d[1, 0, 1]) == 0.0


def test_pair_arap_is_cal_arap_error_of_every_pair():
    """the batched pair form (neighbours of the sampled vertices only, one launch for all pairs) = the reference-shaped
    cal_connectivity_from_points + cal_arap_error per pair (pinned to the reference in tests/test_gpu_arap.py), energy and
    gradient"""
    rng = np.random.default_rng(11)
    B, N, S, K = 4, 6000, 256, 5
    a = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    rot = np.array([[0.96, -0.28, 0.0], [0.28, 0.96, 0.0], [0.0, 0.0, 1.0]], np.float32)
    b_ = (a @ rot.T + 0.02 * rng.normal(size=a.shape)).astype(np.float32)
    pairs = _t(np.stack([a, b_], 1))
    sample = torch.from_numpy(np.stack([rng.choice(N, S) for _ in range(B)])).cuda()
    nbr = pair_connectivity(pairs[:, 0], sample, K=K)
    d_pairs = torch.zeros_like(pairs)
    e = pair_arap(pairs, sample, nbr, d_pairs=d_pairs, grad_scale=0.5)
    for p in range(B):
        nodes = pairs[p].clone().requires_grad_(True)
        res = knn_points(nodes[0:1].detach(), nodes[0:1].detach(), K=K + 1)
        nn_d, nn_i = res.dists[0, :, 1:], res.idx[0, :, 1:].clone()
        nn_i[:, 3:] = torch.where(nn_d[:, 3:] < 0.1 ** 2, nn_i[:, 3:], -torch.ones_like(nn_i[:, 3:]))
        ii = torch.arange(N, device="cuda")[:, None].expand(N, K).reshape(-1)
        jj = nn_i.reshape(-1)
        kk = torch.arange(K, device="cuda")[None].expand(N, K).reshape(-1)
        m = jj != -1
        ref = cal_arap_error(nodes, ii[m], jj[m], kk[m], sample_idx=sample[p])
        ref.backward()
        assert abs(float(e[p]) - float(ref.detach())) <= 1e-4 * abs(float(ref.detach())) + 1e-7
        assert torch.allclose(d_pairs[p], 0.5 * nodes.grad, rtol=2e-4, atol=1e-6 * float(nodes.grad.abs().max()))


def test_l1_loss_and_gradient_in_one_pass():
    F, C, H, W = 3, 5, 37, 41
    row = torch.randn(F, 9, H, W, device="cuda")
    pred = row[:, 2:2 + C]                      # a channel slice of a wider row, as the renderer's images are
    tgt = torch.randn(F, C, H, W, device="cuda")
    tgt[0, 0, 0, :5] = pred[0, 0, 0, :5]        # exact zeros: sign 0
    import ctypes
    g = torch.empty(F, C, H, W, device="cuda")
    s = torch.zeros(1, device="cuda")
    scale = 0.7 / (F * C * H * W)
    L.check(L.lib().splat_l1_loss_grad(F, C * H * W, L.ptr(pred), pred.stride(0), L.ptr(tgt),
                                       scale, L.ptr(g), L.ptr(s), L.stream()))
    p2 = pred.detach().clone().requires_grad_(True)
    (0.7 * (p2 - tgt).abs().mean()).backward()
    assert torch.allclose(g, p2.grad, rtol=1e-6, atol=0) and abs(float(s) - float((pred - tgt).abs().sum())) < 1e-3 * float(s)


# ---------------------------------------------------------------------------------------------------------------------
def _track_frames(o, clock, times1, times2, host, rgb, attrs, extr, W, H, grads, K):
    """oracle: the training frame with track_gs (reference: trainer_fragGS.py:486-512 around render_iter): per pair the
    attribute set is cat(position(ids2), attributes); the gradient of its first three channels goes back through
    get_position(ids2)"""
    N, I = host["position"].shape[0], clock.interval_num
    tot = dict(pos_cubic_node=0.0, rotation=0.0, opacity=0.0, scaling=0.0, rgb=0.0, attrs=0.0, tap=0.0)
    per = []
    zero = lambda *s: np.zeros(s, np.float32)
    for f, (t1, t2) in enumerate(zip(times1, times2)):
        def ev(t):
            seg, d, basis = clock.scalars(t)
            b = np.array(list(basis), np.float32)
            return seg, d, b, o.dynamic_eval_forward(host["position"], host["pos_cubic_node"], host["rotation"], host["rot_poly_feat"],
                                                     host["rot_fourier_feat"], host["opacity"], host["scaling"], seg, d, b[:4], b[4:])
        seg1, d1, b1, (pos1, rot1, opa1, scl1) = ev(t1)
        seg2, d2, b2, (pos2, _, _, _) = ev(t2)
        row = np.concatenate([pos2, attrs], 1).astype(np.float32)
        sets = [dict(feature=rgb, bg=0.2, taps=True), dict(feature="depth", bg=1.0), dict(feature=row, bg=0.0, detach_opacity=True)]
        r = oc.frame(o, pos1, scl1, rot1, opa1, extr, W, H, sets, [g[f] for g in grads], K)
        per.append(r)
        g = r["d"]
        back = lambda seg, d, b, gp, gr, go, gs: o.dynamic_eval_backward(
            (N, 4, I, 3), host["rotation"], host["rot_poly_feat"], host["rot_fourier_feat"], host["opacity"], host["scaling"], seg, d,
            b[:4], b[4:], gp, gr, go, gs)
        _, dcub1, drot, dopa, dscl = back(seg1, d1, b1, g["xyz"].astype(np.float32), g["rotate"].astype(np.float32),
                                          g["opacity"].astype(np.float32), g["scale"].astype(np.float32))
        _, dcub2, _, _, _ = back(seg2, d2, b2, g["feats"][2][:, :3].astype(np.float32), zero(N, 4), zero(N, 1), zero(N, 3))
        tot["pos_cubic_node"] = tot["pos_cubic_node"] + dcub1.astype(np.float64) + dcub2.astype(np.float64)
        tot["rotation"] = tot["rotation"] + drot.astype(np.float64)
        tot["opacity"] = tot["opacity"] + dopa.astype(np.float64)
        tot["scaling"] = tot["scaling"] + dscl.astype(np.float64)
        tot["rgb"] = tot["rgb"] + g["feats"][0]
        tot["attrs"] = tot["attrs"] + g["feats"][2][:, 3:]
        tot["tap"] = tot["tap"] + g["tap"]
    return per, tot


@pytest.mark.parametrize("A", [16, 4, 1])
def test_training_frame_with_track_gs_against_oracle(oracle_mod, A):
    """render_dynamic_sets with the attribute set given as SOURCES [track_gs = position(ids2) per frame | shared attributes], on
    the reference-made dynamic parameters: images, gs_idx and every gradient -- the per-frame gradient of track_gs continued
    through splat_dynamic_positions_batch_backward into the spline segments of the pair frames -- against the oracle chain.
    A = 16: the renderer's own plan (3 | 1 | 19: the tile kernel stages the forward's records); A = 4 / 1: the trainer's
    ['dino_attribute'] / ['mask_attribute'] rows (src/trainer_fragGS.py:657,1214) -- the packing launch takes the row out of the
    forward's records, the SMALL instantiation of the three-set backward runs."""
    g = dict(np.load(os.path.join(GOLD, "dynamic_400x50.npz")))
    clock = FrameClock(int(g["T"]), g["intervals"], int(g["start_frame_id"]), int(g["time_len"]))
    I = clock.interval_num
    names = ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")
    host = {k: np.ascontiguousarray(g[k], np.float32) for k in names}
    N, W, H, K = host["position"].shape[0], 96, 64, 8
    times1, times2 = [0, 5, 24, 25, 44], [45, 1, 44, 0, 49]
    F = len(times1)
    extr = np.eye(4, dtype=np.float32)
    extr[0, 0] = extr[1, 1] = 0.3; extr[2, 2] = 0.1; extr[2, 3] = 2.0
    host["scaling"] = host["scaling"] + 2.0
    rng = np.random.default_rng(8)
    rgb = rng.uniform(size=(N, 3)).astype(np.float32)
    attrs = rng.uniform(-1, 1, size=(N, A)).astype(np.float32)
    gs_ = [rng.normal(size=(F, c, H, W)).astype(np.float32) for c in (3, 1, 3 + A)]
    p = {k: _t(v, k not in ("rot_poly_feat", "rot_fourier_feat", "position")) for k, v in host.items()}
    p["pos_cubic_node"] = to_segment_major(_t(host["pos_cubic_node"]), I).requires_grad_(True)
    t_rgb, t_att = _t(rgb, True), _t(attrs, True)
    # the pairs' positions: [F, 2, N, 3] = (position(ids1), position(ids2)); track_gs is the strided view [:, 1]
    inter = [t for pr in zip(times1, times2) for t in pr]
    pairs = positions_batch(clock, inter, p["position"], p["pos_cubic_node"], cubic_layout=SEGMENT_MAJOR).view(F, 2, N, 3)
    B = FrameBatch(F, N, W, H, 7 + A, "cuda", want_abs=True)
    sets = [dict(feature=t_rgb, bg=0.2, taps=True), dict(feature="depth", bg=1.0),
            dict(feature=[pairs[:, 1], t_att], bg=0.0, detach_opacity=True)]
    o_rgb, o_dep, o_att, ids = B.render_dynamic_sets(
        clock, times1, _t(extr), sets, position=p["position"], pos_cubic_node=p["pos_cubic_node"], rotation=p["rotation"],
        rot_poly_feat=p["rot_poly_feat"], rot_fourier_feat=p["rot_fourier_feat"], opacity=p["opacity"], scaling=p["scaling"],
        cubic_layout=SEGMENT_MAJOR, K=K)
    torch.autograd.backward([o_rgb, o_dep, o_att], [_t(x) for x in gs_])
    torch.cuda.synchronize()
    B.check()
    per, tot = _track_frames(oracle_mod, clock, times1, times2, host, rgb, attrs, extr, W, H, gs_, K)
    assert sum(r["M"] for r in per) > 2000
    got = torch.cat([o_rgb, o_dep, o_att], 1)
    for f, r in enumerate(per):
        c = 0
        for img in r["imgs"]:
            a = got[f, c:c + img.shape[0]].detach().cpu().numpy()
            assert (np.abs(a - img) > (IMG_ATOL + IMG_RTOL * np.abs(img))).mean() < 1e-3, f
            c += img.shape[0]
        assert (ids[f].cpu().numpy() != r["gs_idx"]).any(-1).mean() < 2e-3
    rad = B.radius.cpu().numpy()
    tol = GRAD_RTOL if all((rad[f] == r["radius"]).all() for f, r in enumerate(per)) else 5e-3
    assert_grad(to_gaussian_major(p["pos_cubic_node"].grad).reshape(N, 4, I, 3), tot["pos_cubic_node"], "pos_cubic_node", tol)
    for k in ("rotation", "opacity", "scaling"):
        assert_grad(p[k].grad, tot[k], k, tol)
    assert_grad(t_rgb.grad, tot["rgb"], "rgb", tol)
    assert_grad(t_att.grad, tot["attrs"], "attributes", tol)
    assert_grad(B.tap, tot["tap"], "tap", tol)

    # the same frame with gradient SINKS (what the training step uses): bit-identical parameter gradients
    q = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in p.items()}
    sink = {k: torch.zeros_like(q[k]) for k in ("pos_cubic_node", "rotation", "opacity", "scaling")}
    pr2 = positions_batch(clock, inter, q["position"], q["pos_cubic_node"], cubic_layout=SEGMENT_MAJOR).detach().view(F, 2, N, 3)
    g_pairs = torch.zeros_like(pr2)
    a2 = _t(attrs)
    sink.update({"feature:1": g_pairs[:, 1], "feature:2": torch.zeros_like(a2)})
    r2 = _t(rgb, True)
    sets2 = [dict(feature=r2, bg=0.2, taps=True), dict(feature="depth", bg=1.0), dict(feature=[pr2[:, 1], a2], bg=0.0, detach_opacity=True)]
    o2 = B.render_dynamic_sets(clock, times1, _t(extr), sets2, position=q["position"], pos_cubic_node=q["pos_cubic_node"],
                               rotation=q["rotation"], rot_poly_feat=q["rot_poly_feat"], rot_fourier_feat=q["rot_fourier_feat"],
                               opacity=q["opacity"], scaling=q["scaling"], cubic_layout=SEGMENT_MAJOR, K=K, grad_sink=sink)
    torch.autograd.backward(list(o2[:3]), [_t(x) for x in gs_])
    from splatter_a_video_amd.dynamics import positions_batch_backward
    positions_batch_backward(frame_table(clock, inter, "cuda"), g_pairs.view(2 * F, N, 3), I, SEGMENT_MAJOR, None, sink["pos_cubic_node"])
    assert torch.equal(sink["feature:2"], t_att.grad) and torch.equal(r2.grad, t_rgb.grad)
    for k in ("rotation", "opacity", "scaling"):
        assert torch.equal(sink[k], p[k].grad), k
    assert torch.allclose(sink["pos_cubic_node"], p["pos_cubic_node"].grad, rtol=1e-5, atol=1e-7 * float(p["pos_cubic_node"].grad.abs().max()))
    assert float(g_pairs[:, 0].abs().max()) == 0.0 and float(g_pairs[:, 1].abs().max()) > 0.0


@pytest.mark.parametrize("A", [4, 1])
def test_training_step_with_the_trainers_small_attribute_rows(A):
    """TrainingStep for the trainer's other plans (attrs [N, 4] / [N, 1] behind track_gs: 11 / 8 composited channels): feature
    lists / per-frame sources under a plan whose backward repacks the forward's records (round 6; A = 16 was the only width
    before).  A few steps on a small clip: finite, the loss falls, gradients reach every parameter group."""
    Nn, Ww, Hh, T, F = 2500, 128, 96, 20, 3
    sc = make_scene(Nn, Ww, Hh, F=T, seed=11, sigma_px=3.0)
    clock = FrameClock(T)
    truth = TS.synthetic_video_params(sc, clock, "cuda", attrs=A, seed=12, cubic_sigma=0.01)
    extr = _t(sc.extr)
    lr = dict(TS.REFERENCE_LR, pos_cubic_node=2e-3, shs=2e-2, attrs=2e-2, scaling=1e-2, rotation=5e-3)
    st = TS.TrainingStep(_perturbed(truth, 1), clock, Ww, Hh, F, extr, lr=lr, K=8, arap_samples=128, sample_seed=3)
    t1, t2 = [0, 7, 13], [4, 2, 19]
    gt = TS.render_ground_truth(truth, clock, Ww, Hh, extr, t1, t2)
    before = {k: v.detach().clone() for k, v in st.p.items()}
    losses = []
    for _ in range(12):
        st.step(t1, t2, gt)
        losses.append(st.loss())
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    for k in TS.TRAINABLE:
        assert torch.isfinite(st.p[k]).all() and not torch.equal(st.p[k], before[k]), k


# ---------------------------------------------------------------------------------------------------------------------
def _clip(N, W, H, T, seed):
    sc = make_scene(N, W, H, F=T, seed=seed, sigma_px=3.0)
    clock = FrameClock(T)
    truth = TS.synthetic_video_params(sc, clock, "cuda", attrs=16, seed=seed + 1, cubic_sigma=0.01)
    return sc, clock, truth


def _perturbed(truth, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda t, s: t + s * torch.randn(t.shape, device="cuda", generator=g)
    p = dict(truth)
    p["pos_cubic_node"] = torch.zeros_like(truth["pos_cubic_node"])          # the motion is unknown
    p["shs"] = rn(truth["shs"], 0.25)
    p["attrs"] = rn(truth["attrs"], 0.5)
    p["opacity"] = rn(truth["opacity"], 0.7)
    p["scaling"] = rn(truth["scaling"], 0.15)
    p["rotation"] = rn(truth["rotation"], 0.1)
    return {k: v.clone() for k, v in p.items()}


def test_training_step_fits_a_synthetic_clip_through_densification():
    """The composed step (trainer_fragGS.py:736-790): two dynamic evaluations, the training frame with track_gs, L1 losses,
    K = 5 neighbours + ARAP on every pair, backward, flat Adam, densification statistics -- and every `interval` steps clone /
    split / prune with the Adam moments, Morton reorder and every buffer rebuilt at the new count.  A 20-frame synthetic clip
    rendered from ground-truth Gaussians is fitted from perturbed parameters: the loss falls at least five times, the Gaussian
    count changes at least twice, the gradients stay finite."""
    N, W, H, T, F = 4000, 128, 96, 20, 5
    sc, clock, truth = _clip(N, W, H, T, seed=5)
    extr = _t(sc.extr)
    rng = np.random.default_rng(0)
    cfg = TS.DensifyConfig(interval=50, start_iter=40, stop_iter=160, grad_threshold=5e-4, percent_dense=1e-3, cameras_extent=60.0,
                           min_opacity=0.02, seed=123)     # three rounds of clone + split + prune, then 140 steps at a fixed count
    lr = dict(TS.REFERENCE_LR, pos_cubic_node=2e-3, shs=2e-2, attrs=2e-2, scaling=1e-2, rotation=5e-3)
    st = TS.TrainingStep(_perturbed(truth, 1), clock, W, H, F, extr, lr=lr, densify=cfg, K=8, arap_samples=256)
    gt_cache = {}

    def batch():
        t1 = [int(t) for t in rng.choice(T, F, replace=False)]
        t2 = [int(rng.choice([t for t in range(T) if t != a])) for a in t1]
        key = (tuple(t1), tuple(t2))
        if key not in gt_cache:
            gt_cache[key] = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
        return t1, t2, gt_cache[key]

    losses, counts = [], [st.N]
    for it in range(300):
        t1, t2, gt = batch()
        st.step(t1, t2, gt)
        assert torch.isfinite(st.bucket.flat_grad).all()
        losses.append(st.loss())
        if st.maybe_densify():
            counts.append(st.N)
            st.fb.check()
    first, last = float(np.mean(losses[:3])), float(np.mean(losses[-5:]))
    assert len(counts) >= 3 and len(set(counts)) >= 3, counts         # N changed at least twice
    assert last < first / 5.0, (first, last, counts)
    assert all(np.isfinite(losses))
    assert torch.isfinite(st.bucket.flat_param).all()
    # the Adam moments travelled with the Gaussians: the step count is continuous, the moments are populated
    assert st.opt.t == 300 and float(st.opt.exp_avg_sq.max()) > 0


def test_training_step_phases_are_timed():
    N, W, H, T, F = 3000, 128, 96, 20, 4
    sc, clock, truth = _clip(N, W, H, T, seed=9)
    extr = _t(sc.extr)
    start = _perturbed(truth, 2)
    st = TS.TrainingStep(start, clock, W, H, F, extr, K=8, arap_samples=128, timing=True)
    # set-up put the Gaussians in Morton order of their screen positions; initial_order[i] = the caller's row of Gaussian i
    assert torch.equal(torch.sort(st.initial_order).values, torch.arange(N, device="cuda"))
    assert torch.equal(st.p["rotation"].detach(), start["rotation"][st.initial_order])
    assert TS.TrainingStep(start, clock, W, H, F, extr, K=8, arap_samples=128, spatial_order=False).initial_order is None
    t1, t2 = [0, 3, 7, 12], [5, 1, 19, 2]
    gt = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
    st.step(t1, t2, gt)
    st.step(t1, t2, gt)
    ph = st.phases()
    assert set(ph) == {"model_eval", "knn_arap", "render_forward", "loss", "render_backward", "allreduce_adam", "densify_stats"}
    assert all(v > 0 for v in ph.values())


@pytest.mark.parametrize("owner", [False, True])
def test_opacity_reset_and_learning_rate_schedule_survive_a_rebuild(owner):
    """(owner = True: the owner-sharded optimiser in a single process -- one owner of every block, no collective)"""
    N, W, H, T, F = 2000, 96, 64, 20, 3
    sc, clock, truth = _clip(N, W, H, T, seed=3)
    extr = _t(sc.extr)
    st = TS.TrainingStep(_perturbed(truth, 4), clock, W, H, F, extr, K=4, arap_samples=64, owner_sharded=owner,
                         densify=TS.DensifyConfig(interval=2, start_iter=0, grad_threshold=1e-6, cameras_extent=60.0, min_opacity=0.005, seed=1))
    # (min_opacity below the reset ceiling: the reference relies on the opacities' recovery between a reset and the next prune)
    t1, t2 = [0, 5, 9], [3, 1, 17]
    gt = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
    st.step(t1, t2, gt)
    st.set_lr({"pos_cubic_node": 1.5e-5})
    st.reset_opacity()
    a, b = st.bucket.slices["opacity"]
    assert float(torch.sigmoid(st.p["opacity"].detach()).max()) <= 0.01 + 1e-6 and float(st.opt.full_moments()[0][a:b].abs().max()) == 0.0
    st.step(t1, t2, gt)
    assert st.maybe_densify() and st.N != N
    assert st.opt.lr["pos_cubic_node"] == 1.5e-5 and st.lr["pos_cubic_node"] == 1.5e-5      # the schedule's rate at the new count
    st.step(t1, t2, gt)
    assert torch.isfinite(st.bucket.flat_param).all() and np.isfinite(st.loss())


def test_loss_fused_backward_equals_the_gradient_images():
    """TrainingStep(fused_l1=True): the L1 terms' gradients are derived inside the three-set tile backward from the forward's output
    row and the ground-truth frames (splat_alpha_blending_backward_batch_sets_l1) instead of three splat_l1_loss_grad launches
    whose gradient images the backward reads back.  Same sign rule, same scale: the render-path gradients are bit-identical, the
    loss sums agree to float summation order.  (The spline table also takes the ARAP gradient, scattered with float atomics: two
    runs of one step differ there by ~1e-9.)"""
    N, W, H, T, F = 3000, 128, 96, 20, 4
    sc, clock, truth = _clip(N, W, H, T, seed=11)
    extr = _t(sc.extr)
    start = _perturbed(truth, 3)
    t1, t2 = [0, 3, 7, 12], [5, 1, 19, 2]
    gt = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
    res = []
    for fused in (False, True):
        st = TS.TrainingStep(start, clock, W, H, F, extr, K=8, arap_samples=128, sample_seed=4, fused_l1=fused)
        last = st.step(t1, t2, gt)
        torch.cuda.synchronize()
        res.append((st, {k: float(v) for k, v in last.items()}))
    (a, la), (b, lb) = res
    for name in ("rotation", "opacity", "scaling", "shs", "attrs"):
        assert torch.equal(a.bucket.grad(name), b.bucket.grad(name)), name
        assert float(a.bucket.grad(name).abs().max()) > 0, name
    ga, gb = a.bucket.grad("pos_cubic_node"), b.bucket.grad("pos_cubic_node")
    assert float((ga - gb).abs().max()) <= 1e-6 * float(ga.abs().max())
    assert torch.equal(a.dstate.pos_gradient_accum, b.dstate.pos_gradient_accum)
    for k in ("l1_rgb", "l1_depth", "l1_attr"):
        assert abs(la[k] - lb[k]) <= 1e-5 * abs(la[k]) and la[k] > 0, (k, la[k], lb[k])
