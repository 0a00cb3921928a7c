"""The training step with the reference trainer's loss, dense attribute set against the sparse track term, at the bench's
training-step workload: 300k Gaussians, 854 x 480, 25 pairs of a 50-frame clip, A = 16 attributes,
LossWeights(dssim=0.2, track=2.0, depth=0.0, depth_dpt=1.0, attr=0.0), track targets on a stride grid (about 1000 queries per
pair at the default stride 20).

  dense    TrainingStep(sparse_track=False): the 23-channel row (rgb | depth | track_gs + 16 attributes) is composited and
           replayed for every pixel; the loss reads three of the 19 attribute-set channels at the query pixels
  sparse   TrainingStep(sparse_track=True): rgb + depth in the row (C = 4), track_gs composited at the query pixels only, its
           gradient added to the frame batch's pair records before the Gaussian-side backward
  ordered  TrainingStep(sparse_track=True, ordered_track=True): the sparse step with the ordered backward (no float atomic)
  dense_det / ordered_det   the dense and the ordered sparse step with splat_set_deterministic(1) set around their windows: what
           deterministic training pays for either (the unordered sparse step refuses the flag)

Both legs start from the same perturbed parameters and take the same pairs and targets.  They are timed in alternating rounds
in one process: host clock around a window of consecutive steps with a synchronise on both sides (ms per step; median, minimum
and maximum over the rounds), after warming both up; then one step of each with ``timing=True`` for the phase split and one with
the library's per-kernel events.  One JSON
line (with the commit stamp of tools/stamp.py and the build id) goes to stdout and to --out.

    python tools/train_step_sparse_bench.py [--rounds 5] [--steps 20] [--out profiles/train_step_sparse_track.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from splatter_a_video_amd import _lib as L  # noqa: E402
from splatter_a_video_amd import train_step as TS  # noqa: E402
from splatter_a_video_amd.dynamics import FrameClock  # noqa: E402
from splatter_a_video_amd.synth import make_scene  # noqa: E402
from splatter_a_video_amd.tracks import TrackTargets  # noqa: E402
from stamp import stamp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20, help="steps inside one timed window")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--frames", type=int, default=25)
ap.add_argument("--clip", type=int, default=50)
ap.add_argument("--stride", type=int, default=20, help="query grid stride in pixels (20: 43 x 24 = 1032 queries per pair at 854 x 480)")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "train_step_sparse_track.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("train_step_sparse_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, F, A = args.gaussians, args.width, args.height, args.frames, 16
dev = torch.device("cuda:0")
sc = make_scene(N, W, H, F=args.clip, seed=1234)
clock = FrameClock(sc.F)
truth = TS.synthetic_video_params(sc, clock, dev, attrs=A)
extr = torch.tensor(sc.extr, device=dev)
t1 = [i % sc.F for i in range(F)]
t2 = [int((17 * t + 11) % sc.F) for t in t1]
t2 = [t if t != u else (t + 1) % sc.F for t, u in zip(t2, t1)]
gt = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)

# track targets: the ground truth's own track channels on a stride grid, every query visible
ys, xs = np.meshgrid(np.arange(0, H, args.stride), np.arange(0, W, args.stride), indexing="ij")
q = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.float32)
qi = q.astype(np.int64)
trk = gt["attr"][:, :2].cpu().numpy()
parts = []
for f in range(F):
    t = np.full((q.shape[0], 4), -6.0, np.float32)
    t[:, 0] = (trk[f, 0, qi[:, 1], qi[:, 0]] + 1) * W / 2
    t[:, 1] = (trk[f, 1, qi[:, 1], qi[:, 0]] + 1) * H / 2
    parts.append(TrackTargets.from_reference(q, t, H, W))
gt["tracks"] = TrackTargets.cat(parts).to(dev)
queries_per_pair = int(q.shape[0])

gen = torch.Generator(device=dev).manual_seed(7)
start = {k: v.clone() for k, v in truth.items()}
for k, sg in (("shs", 0.1), ("attrs", 0.2), ("opacity", 0.3), ("scaling", 0.05)):
    start[k] = start[k] + sg * torch.randn(start[k].shape, device=dev, generator=gen)
start["pos_cubic_node"] = torch.zeros_like(start["pos_cubic_node"])
del truth
weights = TS.LossWeights(dssim=0.2, track=2.0, depth=0.0, depth_dpt=1.0, attr=0.0)
lr = {k: 1e-6 for k in TS.REFERENCE_LR}      # small rates keep the scene's statistics put over the run
legs = {name: TS.TrainingStep(start, clock, W, H, F, extr, lr=lr, densify=TS.DensifyConfig(cameras_extent=5.0), K=20, weights=weights,
                              sparse_track=sparse, ordered_track=ordered, sample_seed=3)
        for name, sparse, ordered in (("dense", False, False), ("sparse", True, False), ("ordered", True, True),
                                      ("dense_det", False, False), ("ordered_det", True, True))}
FLAG = {name: name.endswith("_det") for name in legs}      # the deterministic flag is set around these legs' steps only


def window(name, steps):
    st = legs[name]
    L.set_deterministic(FLAG[name])
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            st.step(t1, t2, gt)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    finally:
        L.set_deterministic(False)


for name, st in legs.items():
    window(name, args.warmup)
    st.fb.check()
ms = {name: [] for name in legs}
for _ in range(args.rounds):
    for name in legs:
        ms[name].append(window(name, args.steps))
stat = lambda v: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3),
                  "rounds": len(v)}
rec = {"bench": "train_step_sparse_track", **stamp(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0),
       "gaussians": N, "W": W, "H": H, "pairs": F, "attributes": A, "queries_per_pair": queries_per_pair,
       "loss_weights": "dssim=0.2, track=2.0, depth=0.0, depth_dpt=1.0, attr=0.0", "steps_per_window": args.steps}
for name, st in legs.items():
    L.set_deterministic(FLAG[name])
    st.timing = True
    st.step(t1, t2, gt)
    phases = {k: round(v, 3) for k, v in st.phases().items()}
    st.timing = False
    st.fb.check()
    # per-kernel times of one more step from the library's own events, a pass of its own (the brackets cost host time)
    L.profile_reset()
    L.profile_enable(True)
    st.step(t1, t2, gt)
    torch.cuda.synchronize()
    L.profile_enable(False)
    kern = {}
    for k in ("blend_fwd", "blend_points_bwd", "blend_points_bwd_ord", "blend_points_ord_lists", "blend_points_ord_zero",
              "blend_points_ord_gauss", "blend_points", "blend_pack", "blend_bwd", "gauss_bwd", "track_loss", "track_grad_zero"):
        t_ms, cnt = L.profile_read(k)      # (prefix match: "blend_points" holds both sparse kernels)
        if cnt:
            kern[k] = {"us_per_step": round(t_ms * 1e3, 1), "launches": cnt}
    L.profile_reset()
    L.set_deterministic(False)
    rec[name] = {"ms_per_step": stat(ms[name]), "phases_ms": phases, "kernels_us_per_step": kern, "channels_in_the_row": st.fb.C,
                 "track_loss": float(st.last["track"]), "loss": st.loss()}
med = lambda name: rec[name]["ms_per_step"]["median_ms"]
rec["dense_over_sparse_median"] = round(med("dense") / med("sparse"), 4)
rec["ordered_over_sparse_median"] = round(med("ordered") / med("sparse"), 4)
rec["deterministic_dense_over_ordered_median"] = round(med("dense_det") / med("ordered_det"), 4)
rec["timing"] = ("host clock around a window of consecutive steps, synchronise on both sides, ms per step; windows of the legs "
                 "alternate in one process after warm-up steps of each; phases from device events of one more step per leg; one run "
                 "on a shared machine is a single sample")
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
