"""The 2-D track loss on the GPU (losses.track_loss / track_loss_grad, csrc/loss.hip) against the reference's own functions
(tests/golden/track_loss.npz) and the float32 restatement of test_track_loss_cpu.py; the training step's track term
(LossWeights.track, src/trainer_fragGS.py:528-569)."""
import numpy as np
import pytest
import torch

from splatter_a_video_amd import losses
from splatter_a_video_amd import train_step as TS
from splatter_a_video_amd.tracks import TrackTargets, frame_weights
from test_gpu_ssim import assert_grad_tol
from test_gpu_train_step import _clip, _perturbed, _t
from test_track_loss_cpu import GOLD, restate

pytestmark = pytest.mark.gpu


def _logits(rng, Q, p_hidden=0.25):
    """(occlusion, distance) logits, a fraction hidden; none within 1e-4 of the visibility threshold (the test compares the
    visible count exactly, and the device's sigmoid may round differently from the host's by an ulp)"""
    occ = np.where(rng.random(Q) < p_hidden, rng.uniform(0.5, 5, Q), rng.uniform(-6, -1, Q)).astype(np.float32)
    dist = rng.uniform(-6, 0, Q).astype(np.float32)
    for _ in range(10):
        v = (1 - 1 / (1 + np.exp(-occ.astype(np.float64)))) * (1 - 1 / (1 + np.exp(-dist.astype(np.float64))))
        near = np.abs(v - 0.5) < 1e-4
        if not near.any():
            break
        dist[near] -= 0.01
    return occ, dist


def _random_batch(F, H, W, stride, seed, C=3, shuffle=False, ties=False, hidden=None, Q1=False):
    """a track image [F, C, H, W] on the GPU and per frame (query_xy, target) of a stride grid with noisy targets"""
    rng = np.random.default_rng(seed)
    if ties:
        img = (rng.integers(-64, 64, size=(F, C, H, W)) / 64.0).astype(np.float32)
    else:
        img = rng.uniform(-1, 1, size=(F, C, H, W)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    grid = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.float32)
    pairs = []
    for f in range(F):
        q = grid[:1] + np.float32(0.5) if Q1 else grid.copy()
        Q = q.shape[0]
        pi = q.astype(np.int64)
        X = ((img[f, 0] + np.float32(1)) * np.float32(W)) / np.float32(2)
        Y = ((img[f, 1] + np.float32(1)) * np.float32(H)) / np.float32(2)
        t = np.zeros((Q, 4), np.float32)
        if ties:
            off = rng.integers(-2, 3, size=(Q, 2)) / 4.0
            off[rng.random(Q) < 0.3] = 0.0               # pred == gt
        else:
            off = rng.normal(0, 3.0, size=(Q, 2))
            off[rng.random(Q) < 0.03] *= 20.0
        t[:, 0] = X[pi[:, 1], pi[:, 0]] + off[:, 0]
        t[:, 1] = Y[pi[:, 1], pi[:, 0]] + off[:, 1]
        t[:, 2], t[:, 3] = _logits(rng, Q)
        if hidden is not None and f in hidden:
            t[:, 2] = 6.0                               # every query occluded
        if shuffle:
            perm = rng.permutation(Q)
            q, t = q[perm] + rng.uniform(0, 0.9, size=q.shape).astype(np.float32), t[perm]
        pairs.append((q, t))
    return torch.from_numpy(img), pairs


def _targets(pairs, H, W):
    return TrackTargets.cat([TrackTargets.from_reference(q, t, H, W) for q, t in pairs]).to("cuda")


def _restated(img_cpu, tt_cpu_parts, w, H, W, quantile):
    """per frame (loss, n, s) and the gradient of the mean over frames w.r.t. the image, float32 on the CPU"""
    img = img_cpu.clone().requires_grad_(True)
    res = [restate(img[f], p.pixels, p.targets, w[f], H, W, quantile) for f, p in enumerate(tt_cpu_parts)]
    mean = torch.stack([r[0] for r in res]).mean()
    (g,) = torch.autograd.grad(mean, [img])
    return [float(r[0].detach()) for r in res], [(r[1], r[2]) for r in res], g


def _check_case(img, pairs, H, W, w, quantile=0.98, view=None):
    """the kernel against the restatement: counts exact, losses rtol 1e-5, the gradient within the project's tolerance"""
    F = img.shape[0]
    parts = [TrackTargets.from_reference(q, t, H, W) for q, t in pairs]
    tt = TrackTargets.cat(parts).to("cuda")
    dimg = img.cuda() if view is None else view
    per = torch.empty(F, device="cuda")
    counts = torch.empty(F, 2, dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, device="cuda")
    grad = torch.full(dimg.shape, 7.0, device="cuda")
    losses.track_loss_grad(dimg, tt, w, quantile, 1.0, grad, per_frame=per, loss_slot=slot, counts=counts)
    want, want_counts, want_g = _restated(img, parts, w, H, W, quantile)
    assert [tuple(c) for c in counts.cpu().tolist()] == want_counts
    np.testing.assert_allclose(per.cpu().numpy(), np.array(want, np.float32), rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(float(slot), float(np.mean(want)), rtol=1e-5, atol=1e-12)
    assert_grad_tol(grad, want_g, "track gradient")
    assert torch.equal(grad.cpu() != 0, want_g != 0)
    return per, counts, grad


def test_track_loss_matches_the_reference_fixture():
    g = np.load(GOLD)
    cases = ["grid", "shuffled", "ties", "nan"]
    G = lambda c, k: g[f"{c}_{k}"]
    H, W = G("grid", "track").shape[-2:]
    tt = TrackTargets.cat([TrackTargets.from_reference(G(c, "query_xy"), G(c, "target"), H, W) for c in cases]).to("cuda")
    w = frame_weights([int(G(c, "ids1")) for c in cases], [int(G(c, "ids2")) for c in cases], int(G("grid", "num_imgs")))
    img = torch.from_numpy(np.concatenate([G(c, "track") for c in cases])).cuda().requires_grad_(True)
    per = torch.empty(len(cases), device="cuda")
    losses.track_loss_grad(img.detach(), tt, w, per_frame=per)
    for k, c in enumerate(cases):
        np.testing.assert_allclose(float(per[k]), float(G(c, "loss")), rtol=1e-5)
    loss = losses.track_loss(img, tt, w)
    np.testing.assert_allclose(float(loss.detach()), np.mean([float(G(c, "loss")) for c in cases]), rtol=1e-5)
    (d,) = torch.autograd.grad(loss * len(cases), [img])    # the mean over the pairs, times their number: each pair's own
    for k, c in enumerate(cases):
        assert_grad_tol(d[k], torch.from_numpy(G(c, "grad")[0]), c)
    # one pair at a time through the autograd Function
    for c in cases:
        one = torch.from_numpy(G(c, "track")).cuda().requires_grad_(True)
        t1 = TrackTargets.from_reference(G(c, "query_xy"), G(c, "target"), H, W).to("cuda")
        l1 = losses.track_loss(one, t1, frame_weights([int(G(c, "ids1"))], [int(G(c, "ids2"))], int(G(c, "num_imgs"))))
        l1.backward()
        np.testing.assert_allclose(float(l1.detach()), float(G(c, "loss")), rtol=1e-5)
        assert_grad_tol(one.grad, torch.from_numpy(G(c, "grad")), c)


def test_track_loss_full_size_batch():
    """F = 25 frames of 854 x 480, a stride-4 query grid: 25 680 queries per frame"""
    F, H, W = 25, 480, 854
    img, pairs = _random_batch(F, H, W, 4, seed=1)
    assert pairs[0][0].shape[0] == 25680
    rng = np.random.default_rng(3)
    t1 = rng.integers(0, 40, F)
    w = frame_weights(t1, rng.integers(0, 40, F), 40)
    _check_case(img, pairs, H, W, w)


@pytest.mark.parametrize("name", ["q1", "hidden_frame", "quantile0", "quantile1", "shuffled", "ties", "channel_slice",
                                  "nan_frame"])
def test_track_loss_edge_cases(name):
    H, W, F = 60, 90, 4
    kw = dict(q1=dict(Q1=True), hidden_frame=dict(hidden={1}), shuffled=dict(shuffle=True), ties=dict(ties=True)).get(name, {})
    img, pairs = _random_batch(F, H, W, 3, seed=sum(map(ord, name)), **kw)
    w = frame_weights([0, 2, 5, 9], [3, 2, 1, 20], 24)
    q = {"quantile0": 0.0, "quantile1": 1.0}.get(name, 0.98)
    view = None
    if name == "nan_frame":         # a diverged pixel at a visible query of frame 2: the reference's loss there is 0
        q0, t0 = pairs[2]
        vis = (1 - 1 / (1 + np.exp(-t0[:, 2].astype(np.float64)))) * (1 - 1 / (1 + np.exp(-t0[:, 3].astype(np.float64)))) > 0.5
        x, y = q0[np.nonzero(vis)[0][0]].astype(int)
        img[2, 1, y, x] = float("nan")
    if name == "channel_slice":       # the track channels inside a wider row [F, 23, H, W], read in place
        row = torch.randn(F, 23, H, W, device="cuda")
        row[:, 4:7] = img.cuda()
        view = row[:, 4:7]
        assert not view.is_contiguous()
    per, counts, grad = _check_case(img, pairs, H, W, w, q, view)
    if name == "nan_frame":
        assert int(counts[2, 0]) > 0 and int(counts[2, 1]) == 0 and float(per[2]) == 0.0 and float(grad[2].abs().max()) == 0.0
        assert int(counts[1, 1]) > 0 and float(per[1]) > 0.0
    if name == "hidden_frame":
        assert counts[1].tolist() == [0, 0] and float(per[1]) == 0.0 and float(grad[1].abs().max()) == 0.0
    if name == "q1":
        assert counts[:, 1].tolist() == counts[:, 0].tolist() and int(counts[:, 0].max()) <= 1
    if name == "quantile1":
        assert counts[:, 1].tolist() == counts[:, 0].tolist()
    if name == "ties":
        assert int(counts[:, 1].sum()) > 0


def test_track_loss_accumulates_and_leaves_other_pixels():
    H, W, F = 48, 64, 2
    img, pairs = _random_batch(F, H, W, 4, seed=9)
    tt = _targets(pairs, H, W)
    w = frame_weights([0, 1], [4, 9], 12)
    dimg = img.cuda()
    g0 = torch.empty_like(dimg)
    losses.track_loss_grad(dimg, tt, w, 0.98, 2.5, g0)
    base = torch.randn_like(dimg)
    g1 = base.clone()
    losses.track_loss_grad(dimg, tt, w, 0.98, 2.5, g1, accumulate=True)
    assert torch.equal(g1, base + g0)
    assert float(g0[:, 2].abs().max()) == 0.0


def test_track_loss_skips_duplicate_and_unsorted_pixels():
    """a raw batch that bypasses TrackTargets.from_reference: a query whose pixel index is not above the frame's previous one
    (a duplicate, or out of order) is skipped like an out-of-range one -- the result equals the batch without those entries,
    and the gradient's read-modify-write never sees two queries of one pixel (bit-identical from run to run)"""
    H, W, F = 48, 64, 2
    img, pairs = _random_batch(F, H, W, 4, seed=31)
    clean = [TrackTargets.from_reference(q, t, H, W) for q, t in pairs]
    # frame 0: entry 5 repeated right after itself; frame 1: entries 7 and 8 swapped (8 is then below 7: skipped) and a
    # negative index appended
    p0, t0 = clean[0].pixels, clean[0].targets
    p1, t1 = clean[1].pixels.clone(), clean[1].targets
    raw_p0 = torch.cat([p0[:6], p0[5:6], p0[6:]])
    raw_t0 = torch.cat([t0[:6], t0[5:6], t0[6:]])
    raw_p1 = torch.cat([p1[:7], p1[8:9], p1[7:8], p1[9:], torch.tensor([-3], dtype=torch.int32)])
    raw_t1 = torch.cat([t1[:7], t1[8:9], t1[7:8], t1[9:], t1[:1]])
    counts = [raw_p0.numel(), raw_p1.numel()]
    raw = TrackTargets(torch.tensor([0, counts[0], sum(counts)]), torch.cat([raw_p0, raw_p1]), torch.cat([raw_t0, raw_t1]), H, W,
                       counts).to("cuda")
    # frame 1 keeps the swapped-in entry 8 (above entry 6) and skips entry 7 behind it, and the negative index
    ref = TrackTargets.cat([clean[0], TrackTargets(torch.tensor([0, p1.numel() - 1]),
                                                   torch.cat([p1[:7], p1[8:9], p1[9:]]), torch.cat([t1[:7], t1[8:9], t1[9:]]),
                                                   H, W, [p1.numel() - 1])]).to("cuda")
    w = frame_weights([0, 3], [5, 1], 10)
    dimg = img.cuda()
    outs = []
    for tt in (raw, raw, ref):
        g = torch.empty_like(dimg)
        per = torch.empty(F, device="cuda")
        cnt = torch.empty(F, 2, dtype=torch.int32, device="cuda")
        losses.track_loss_grad(dimg, tt, w, 0.98, 1.0, g, per_frame=per, counts=cnt)
        outs.append((g, per, cnt))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert torch.equal(outs[0][2], outs[2][2])
    # the same terms, summed by other threads (the skipped entries shift the rest): equal to rounding
    np.testing.assert_allclose(outs[0][1].cpu().numpy(), outs[2][1].cpu().numpy(), rtol=1e-6)
    assert_grad_tol(outs[0][0], outs[2][0], "gradient without the malformed entries")
    assert torch.equal(outs[0][0] != 0, outs[2][0] != 0)


def test_track_loss_is_deterministic_and_graph_capturable():
    H, W, F = 120, 214, 6
    img, pairs = _random_batch(F, H, W, 2, seed=21, ties=True)
    tt = _targets(pairs, H, W)
    w = frame_weights(list(range(F)), [5, 0, 1, 2, 3, 4], F).cuda()
    dimg = img.cuda()

    def run():
        g = torch.empty_like(dimg)
        per = torch.empty(F, device="cuda")
        cnt = torch.empty(F, 2, dtype=torch.int32, device="cuda")
        slot = torch.zeros(1, device="cuda")
        losses.track_loss_grad(dimg, tt, w, 0.98, 1.0, g, per_frame=per, loss_slot=slot, counts=cnt)
        return g, per, cnt, slot

    r1, r2 = run(), run()
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(static, r1))


# ------------------------------------------------------------------------------------------------------------ training step
def _step_tracks(gt, stride, seed, noise):
    """track targets of the step's pairs sampled from a ground-truth render's track channels on a stride grid"""
    attr = gt["attr"]
    F, _, H, W = attr.shape
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    q = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.float32)
    a = attr.detach().cpu().numpy()
    parts = []
    for f in range(F):
        X = ((a[f, 0] + np.float32(1)) * np.float32(W)) / np.float32(2)
        Y = ((a[f, 1] + np.float32(1)) * np.float32(H)) / np.float32(2)
        t = np.full((q.shape[0], 4), -6.0, np.float32)
        t[:, 0] = X[q[:, 1].astype(int), q[:, 0].astype(int)] + noise * rng.normal(size=q.shape[0])
        t[:, 1] = Y[q[:, 1].astype(int), q[:, 0].astype(int)] + noise * rng.normal(size=q.shape[0])
        parts.append(TrackTargets.from_reference(q, t, H, W))
    return TrackTargets.cat(parts).to("cuda")


class _AutogradTrack(TS.TrainingStep):
    """the track term's gradient by torch autograd through the float32 restatement (on the GPU)"""

    def _track_loss_grad(self, pred, tracks, weights, grad, slot):
        p = pred.detach().clone().requires_grad_(True)
        o = np.concatenate([[0], np.cumsum(tracks.counts)])
        ls = [restate(p[f], tracks.pixels[o[f]:o[f + 1]], tracks.targets[o[f]:o[f + 1]], weights[f], self.H, self.W,
                      self.w.track_quantile)[0] for f in range(self.F)]
        mean = torch.stack(ls).mean()
        (g,) = torch.autograd.grad(self.w.track * mean, [p])
        grad.copy_(g)
        slot += mean.detach()


def test_training_step_track_gradients_match_autograd():
    N, W, H, T, F = 3000, 128, 96, 20, 4
    sc, clock, truth = _clip(N, W, H, T, seed=11)
    extr = _t(sc.extr)
    start = _perturbed(truth, 3)
    t1, t2 = [0, 3, 7, 12], [5, 1, 19, 2]
    gt = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
    gt["tracks"] = _step_tracks(gt, 4, seed=2, noise=0.5)
    w = TS.LossWeights(track=2.0)
    res = []
    for cls in (TS.TrainingStep, _AutogradTrack):
        st = cls(start, clock, W, H, F, extr, K=8, arap_samples=128, sample_seed=4, weights=w)
        last = st.step(t1, t2, gt)
        torch.cuda.synchronize()
        res.append((st, last))
    (a, la), (b, lb) = res
    assert set(la) == {"l1_rgb", "l1_depth", "l1_attr", "arap", "track"} == set(lb)
    for name in ("pos_cubic_node", "rotation", "opacity", "scaling", "shs", "attrs"):
        assert float(a.bucket.grad(name).abs().max()) > 0, name
        assert_grad_tol(a.bucket.grad(name), b.bucket.grad(name), name)
    np.testing.assert_allclose(float(la["track"]), float(lb["track"]), rtol=1e-5)
    assert float(la["track"]) > 0
    # the attribute L1 covers the A attribute channels only
    pred = TS.render_ground_truth(start, clock, W, H, extr, t1, t2)["attr"]
    want = float((pred[:, 3:] - gt["attr"][:, 3:]).abs().mean())
    np.testing.assert_allclose(float(la["l1_attr"]), want, rtol=1e-4)
    assert abs(a.loss() - (float(la["l1_rgb"]) + float(la["l1_depth"]) + float(la["l1_attr"]) + 1e-3 * float(la["arap"])
                           + 2.0 * float(la["track"]))) <= 1e-6 * max(1.0, abs(a.loss()))
    with pytest.raises(ValueError):
        a.step(t1, t2, {k: v for k, v in gt.items() if k != "tracks"})


def test_training_step_track_term_converges():
    N, W, H, T, F = 4000, 128, 96, 20, 5
    sc, clock, truth = _clip(N, W, H, T, seed=5)
    extr = _t(sc.extr)
    rng = np.random.default_rng(0)
    lr = dict(TS.REFERENCE_LR, pos_cubic_node=2e-3)
    st = TS.TrainingStep(_perturbed(truth, 1), clock, W, H, F, extr, lr=lr, K=8, arap_samples=256,
                         weights=TS.LossWeights(rgb=0.0, depth=0.0, attr=0.0, track=2.0))
    gts = {}
    track = []
    for it in range(150):
        t1 = [int(t) for t in rng.choice(T, F, replace=False)]
        t2 = [int(rng.choice([t for t in range(T) if t != x])) for x in t1]
        key = (tuple(t1), tuple(t2))
        if key not in gts:
            gts[key] = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
            gts[key]["tracks"] = _step_tracks(gts[key], 4, seed=len(gts), noise=0.0)
        last = st.step(t1, t2, gts[key])
        track.append(float(last["track"]))
    assert all(np.isfinite(track))
    first, final = float(np.mean(track[:3])), float(np.mean(track[-5:]))
    assert final < first / 3.0, (first, final)
