"""The 2-D track loss at the training step's size (25 frames of 854 x 480, a stride-4 query grid: 25 680 queries per frame): the
HIP path (splat_track_loss_grad: loss only, loss + gradient image, losses.track_loss forward + backward) against the float32
eager restatement of tests/test_track_loss_cpu.py on the same GPU, and TrainingStep(timing=True) on bench.py's training scene
with LossWeights.track = 0 (fused and unfused L1) and 2.0 (GPU box).  HIP events around `--repeat` iterations after `--warmup`;
prints one JSON line (and writes it with --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import losses
from splatter_a_video_amd import train_step as TS
from splatter_a_video_amd.dynamics import FrameClock
from splatter_a_video_amd.synth import make_scene
from splatter_a_video_amd.tracks import TrackTargets, frame_weights
from test_track_loss_cpu import restate


def timed(fn, warmup, repeat):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeat):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeat


def grid_tracks(track, stride, seed, noise=2.0):
    """TrackTargets of a stride grid: targets = the image's own denormalised prediction + noise, TAPIR-like logits"""
    F, _, H, W = track.shape
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    q = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.float32)
    a = track[:, :2].detach().cpu().numpy()
    parts = []
    for f in range(F):
        X = ((a[f, 0] + np.float32(1)) * np.float32(W)) / np.float32(2)
        Y = ((a[f, 1] + np.float32(1)) * np.float32(H)) / np.float32(2)
        t = np.empty((q.shape[0], 4), np.float32)
        t[:, 0] = X[q[:, 1].astype(int), q[:, 0].astype(int)] + noise * rng.normal(size=q.shape[0])
        t[:, 1] = Y[q[:, 1].astype(int), q[:, 0].astype(int)] + noise * rng.normal(size=q.shape[0])
        t[:, 2] = rng.normal(-3, 2, size=q.shape[0])
        t[:, 3] = rng.normal(-3, 2, size=q.shape[0])
        parts.append(TrackTargets.from_reference(q, t, H, W))
    return TrackTargets.cat(parts).to(track.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--step-repeat", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_loss_probe needs a GPU")
    dev = torch.device("cuda:0")
    F, H, W = a.frames, 480, 854
    gen = torch.Generator(device=dev).manual_seed(0)
    row = torch.rand(F, 23, H, W, device=dev, generator=gen) * 2 - 1       # the step's attribute row; track_gs = channels 0..2
    track = row[:, :3]
    tt = grid_tracks(track, 4, seed=1)
    w = frame_weights(list(range(F)), [(7 * t + 3) % 50 for t in range(F)], 50).to(dev)
    rec = {"build_id": L.build_id(), "frames": F, "size": [H, W], "queries_per_frame": tt.counts[0], "warmup": a.warmup,
           "repeat": a.repeat}
    per = torch.empty(F, device=dev)
    g = torch.empty(F, 3, H, W, device=dev)
    p = track.clone().requires_grad_(True)

    def autograd_fn():
        torch.autograd.grad(losses.track_loss(p, tt, w), [p])

    def eager():
        img = track.detach().clone().requires_grad_(True)
        o = np.concatenate([[0], np.cumsum(tt.counts)])
        ls = [restate(img[f], tt.pixels[o[f]:o[f + 1]], tt.targets[o[f]:o[f + 1]], w[f], H, W)[0] for f in range(F)]
        torch.autograd.grad(torch.stack(ls).mean(), [img])

    r = {"loss_only_ms": timed(lambda: losses.track_loss_grad(track, tt, w, per_frame=per), a.warmup, a.repeat),
         "loss_and_grad_ms": timed(lambda: losses.track_loss_grad(track, tt, w, 0.98, 2.0, g, per_frame=per), a.warmup, a.repeat),
         "grad_accumulate_ms": timed(lambda: losses.track_loss_grad(track, tt, w, 0.98, 2.0, g, accumulate=True), a.warmup,
                                     a.repeat),
         "track_loss_fwd_bwd_ms": timed(autograd_fn, a.warmup, a.repeat),
         "eager_fwd_bwd_ms": timed(eager, 1, 3)}
    r = {k: round(v, 4) for k, v in r.items()}
    r["speedup_vs_eager"] = round(r["eager_fwd_bwd_ms"] / r["track_loss_fwd_bwd_ms"], 1)
    counts = torch.empty(F, 2, dtype=torch.int32, device=dev)
    losses.track_loss_grad(track, tt, w, per_frame=per, counts=counts)
    o = np.concatenate([[0], np.cumsum(tt.counts)])
    want = [restate(track[f], tt.pixels[o[f]:o[f + 1]], tt.targets[o[f]:o[f + 1]], w[f], H, W) for f in range(F)]
    got = per.cpu().numpy()
    r["max_rel_loss_diff_vs_eager"] = float(max(abs(got[f] - float(want[f][0])) / float(want[f][0]) for f in range(F)))
    r["counts_equal"] = [tuple(c) for c in counts.cpu().tolist()] == [(x[1], x[2]) for x in want]
    rec["kernel"] = r
    del row, track, p, g
    torch.cuda.empty_cache()
    # the training step: bench.py --train-step's scene and frames, with and without the term
    sc = make_scene(a.gaussians, W, H, F=50, C=0, seed=1234)
    clock = FrameClock(sc.F)
    truth = TS.synthetic_video_params(sc, clock, dev, attrs=16)
    extr = torch.tensor(sc.extr, device=dev)
    t1 = list(range(F))
    t2 = [int((17 * t + 11) % sc.F) for t in t1]
    t2 = [t if t != u else (t + 1) % sc.F for t, u in zip(t2, t1)]
    gts = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
    gts["tracks"] = grid_tracks(gts["attr"][:, :3], 4, seed=2, noise=1.0)
    g2 = torch.Generator(device=dev).manual_seed(7)
    start = {k: v.clone() for k, v in truth.items()}
    for k, sg in (("shs", 0.1), ("attrs", 0.2), ("opacity", 0.3), ("scaling", 0.05)):
        start[k] = start[k] + sg * torch.randn(start[k].shape, device=dev, generator=g2)
    start["pos_cubic_node"] = torch.zeros_like(start["pos_cubic_node"])
    del truth
    lr = {k: 1e-6 for k in TS.REFERENCE_LR}
    steps = {}
    for name, weights, fused in (("track0_fused", TS.LossWeights(), True), ("track0_unfused", TS.LossWeights(), False),
                                 ("track2", TS.LossWeights(track=2.0), True)):
        st = TS.TrainingStep(start, clock, W, H, F, extr, lr=lr, K=20, weights=weights, timing=True, fused_l1=fused)
        st.step(t1, t2, gts)
        acc, tot = [], []
        for _ in range(a.step_repeat):
            st.step(t1, t2, gts)
            ph = st.phases()
            acc.append(ph["loss"])
            tot.append(sum(ph.values()))
        steps[name] = {"loss_phase_ms": round(sorted(acc)[len(acc) // 2], 4), "step_ms": round(sorted(tot)[len(tot) // 2], 3),
                       "loss": st.loss()}
        if "track" in st.last:
            steps[name]["track"] = float(st.last["track"])
        del st
        torch.cuda.empty_cache()
    steps["step_added_ms"] = round(steps["track2"]["step_ms"] - steps["track0_fused"]["step_ms"], 3)
    rec["train_step"] = steps
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
