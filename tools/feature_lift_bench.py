"""Feature lifting (splatter_a_video_amd.lift, DESIGN "Feature lifting") against the route the project offered before it, on the
scene of the other tools: 300k Gaussians, 854 x 480, 25 frames of a 50-frame clip, maps of D = 64 and D = 1 channels.

  lift      FeatureLift.add(times, maps): per batch of frames one preprocess, one binning, one sort, then per chunk of 32
            channels splat_blend_lift_batch + splat_lift_fold (num and den)
  backward  FrameBatch.render_dynamic_sets(wide=feature [N, D]) forward plus backward with dL_dout = maps on the wide output
            (num only): forward of the row and of every chunk, the chunk's tile backward (replay, dL/dalpha), the fold and the
            Gaussian-side walk

Before anything is timed the two routes must agree: num within the gradient bound of the GPU tests (tests/test_gpu_lift.py, bound
1).  Then whole clips alternate in one process, each timed with device events after a warm-up clip of each route; ms per frame =
clip time / frames, median (min .. max) over the windows.  One JSON record (commit stamp of tools/stamp.py, build id) goes to
stdout and to --out.

    python tools/feature_lift_bench.py [--windows 5] [--out profiles/feature_lift.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from splatter_a_video_amd import _lib as L  # noqa: E402
from splatter_a_video_amd import train_step as TS  # noqa: E402
from splatter_a_video_amd.dynamics import SEGMENT_MAJOR, FrameClock, to_segment_major  # noqa: E402
from splatter_a_video_amd.frames import FrameBatch  # noqa: E402
from splatter_a_video_amd.lift import FeatureLift  # noqa: E402
from splatter_a_video_amd.synth import make_scene  # noqa: E402
from stamp import stamp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--clip", type=int, default=50)
ap.add_argument("--frames", type=int, default=25)
ap.add_argument("--frames-per-batch", type=int, default=5)
ap.add_argument("--widths", type=int, nargs="+", default=[64, 1])
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "feature_lift.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("feature_lift_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, T, FB = args.gaussians, args.width, args.height, args.frames, args.frames_per_batch
if T % FB:
    sys.exit("--frames must be a multiple of --frames-per-batch (the backward route has no padded batch)")
dev = torch.device("cuda:0")
sc = make_scene(N, W, H, F=args.clip, seed=1234)
clock = FrameClock(sc.F)
I = clock.interval_num
par = TS.synthetic_video_params(sc, clock, dev)
par["pos_cubic_node"] = to_segment_major(par["pos_cubic_node"], I)
extr = torch.tensor(sc.extr, device=dev)
geo = {k: par[k] for k in ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")}
times = [(2 * i) % sc.F for i in range(T)]
gen = torch.Generator(device=dev).manual_seed(7)
rgb = torch.rand(N, 3, device=dev, generator=gen)


def routes(D):
    maps = torch.randn(T, D, H, W, device=dev, generator=gen)
    lift = FeatureLift(geo, clock, extr, W, H, D, frames_per_batch=FB, cubic_layout=SEGMENT_MAJOR)
    fb = FrameBatch(FB, N, W, H, 3, dev)
    feat = torch.zeros(N, D, device=dev, requires_grad=True)

    def leg_lift():
        lift.num.zero_()
        lift.den.zero_()
        lift.add(times, maps)
        return lift.num

    def leg_backward():
        feat.grad = None
        for b0 in range(0, T, FB):
            out = fb.render_dynamic_sets(clock, times[b0:b0 + FB], extr, [dict(feature=rgb, bg=0.0, taps=True)],
                                         wide=dict(feature=feat, bg=0.0, detach_opacity=True), cubic_layout=SEGMENT_MAJOR, **geo)
            torch.autograd.backward([out[1]], [maps[b0:b0 + FB]])
        return feat.grad

    return lift, fb, {"lift": leg_lift, "backward": leg_backward}


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / T


stat = lambda v: {"median_ms_per_frame": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3),
                  "windows": len(v)}
rec = {"bench": "feature_lift", **stamp(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "gaussians": N, "W": W, "H": H,
       "frames": T, "frames_per_batch": FB, "widths": {}}
for D in args.widths:
    lift, fb, legs = routes(D)
    # ---- the two routes agree (bound 1), before anything is timed: one clip of each, the warm-up
    a, b = legs["lift"]().double(), legs["backward"]().double()
    torch.cuda.synchronize()
    lim = 2.0 * (2e-3 * b.abs() + 1e-4 * b.abs().max())
    worst = float(((a - b).abs() / lim).max())
    assert worst <= 1.0, f"D = {D}: num is {worst:.2f} x the gradient bound away from the backward route"
    ms = {name: [] for name in legs}
    for _ in range(args.windows):
        for name, fn in legs.items():
            ms[name].append(window(fn))
    r = {"legs": {name: stat(v) for name, v in ms.items()}, "worst_error_over_bound": round(worst, 4),
         "max_pairs_per_frame": int(lift.fb.check()), "regrows": lift.regrows, "lift_record_bytes": int(lift._records().numel() * 4)}
    r["backward_over_lift"] = round(r["legs"]["backward"]["median_ms_per_frame"] / r["legs"]["lift"]["median_ms_per_frame"], 3)
    # per-kernel times of one more lifted clip from the library's own events (a pass of its own)
    L.profile_reset()
    L.profile_enable(True)
    legs["lift"]()
    torch.cuda.synchronize()
    L.profile_enable(False)
    kern = {}
    for k in ("frame_preprocess_fwd_layer", "bin_count", "bin_scatter", "tile_sort", "blend_lift", "lift_fold"):
        t_ms, cnt = L.profile_read(k)
        if cnt:
            kern[k] = {"us_per_frame": round(t_ms * 1e3 / T, 2), "launches": cnt}
    L.profile_reset()
    r["lift_kernels"] = kern
    rec["widths"][str(D)] = r
    del lift, fb, legs, a, b
    torch.cuda.empty_cache()
rec["timing"] = ("device events around one whole clip, synchronise on both sides, ms per frame = clip time / frames; the two routes' "
                 "clips alternate in one process after the agreement check (one clip of each: the warm-up); median (min .. max) of "
                 "the windows; the lift's clip includes one host synchronisation per batch (the pair counts); one run on a shared "
                 "machine is a single sample")
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
