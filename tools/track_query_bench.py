"""Point tracking at the c2 scene (300k Gaussians, 854 x 480, dynamic parameters of train_step.synthetic_video_params): T = 50
target frames, Q = 1024 query pixels of frame 0.

  native    tracking.track_pixels: preprocess + sort of the query frame, splat_track_flow_rows, ONE sparse walk
            (splat_alpha_blending_points_forward) of a 150-channel row per query
  composed  the same answer from the operators that existed before it, per target frame: evaluate, project_point_ortho,
            dense alpha_blending of the 2-channel flow, F.grid_sample at the queries (the query frame's preprocess + sort once)

Both are timed in alternating rounds in one process with device events around a window of consecutive calls (--calls of the native
route, a fifth as many of the composed one: a single native call is under a millisecond) and a synchronise behind it (ms per call;
median and minimum over the rounds), after warming both up; the kernels' own time comes from a separate pass with the library's per-kernel
events switched on.  The two routes' tracks are compared.  One JSON record (with the build id) goes to --out.

    python tools/track_query_bench.py [--rounds 10] [--out profiles/track_query.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dptr.gs as gs  # noqa: E402
from splatter_a_video_amd import _lib as L  # noqa: E402
from splatter_a_video_amd.dynamics import FrameClock, evaluate, frame_preprocess  # noqa: E402
from splatter_a_video_amd.synth import make_scene  # noqa: E402
from splatter_a_video_amd.tracking import track_pixels  # noqa: E402
from splatter_a_video_amd.train_step import synthetic_video_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--calls", type=int, default=20, help="calls inside one timed window of the native route (a single call is under a millisecond)")
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--frames", type=int, default=50)
ap.add_argument("--queries", type=int, default=1024)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "track_query.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("track_query_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, T, Q = args.gaussians, 854, 480, args.frames, args.queries
NEAREST, EXTENT = 0.01, 1.3
dev = torch.device("cuda:0")
sc = make_scene(N, W, H, seed=1234)
clock = FrameClock(T)
p = synthetic_video_params(sc, clock, dev)
extr = torch.tensor(sc.extr, device=dev)
times = list(range(T))
rng = np.random.default_rng(7)
px = torch.tensor(rng.uniform(0, [W, H], size=(Q, 2)).astype(np.float32), device=dev)
dyn = {k: p[k] for k in ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")}


def native():
    return track_pixels(dyn, clock, 0, px, times, extr, W, H, nearest=NEAREST, extent=EXTENT).tracks


@torch.no_grad()
def composed():
    uv, depth, conic, radius, tiles, opa = frame_preprocess(clock, 0, extr, W, H, nearest=NEAREST, extent=EXTENT, **dyn)
    idx, tr = gs.sort_gaussian(uv, depth, W, H, radius, tiles)
    grid = (px / torch.tensor([W, H], dtype=torch.float32, device=dev) * 2 - 1.0)[None, :, None, :]     # normalize_coords
    out = []
    for t in times:
        pos_t = evaluate(clock, t, position=dyn["position"], pos_cubic_node=dyn["pos_cubic_node"])[0]
        uv_t, _ = gs.project_point_ortho(pos_t, extr, W, H, nearest=NEAREST, extent=EXTENT)
        img = gs.alpha_blending(uv, conic, opa, uv_t - uv, idx, tr, 0.0, W, H)
        flow = F.grid_sample(img[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        out.append(px + flow[0, :, :, 0].permute(1, 0))
    return torch.stack(out)


def timed(fn, calls=1):
    """ms per call of `calls` consecutive calls inside one window"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


for _ in range(2):      # warm up every shape of the timed window
    a, b = native(), composed()
torch.cuda.synchronize()
diff = float((a - b).abs().max())
ms = {"native": [], "composed": []}
for _ in range(args.rounds):
    ms["native"].append(timed(native, args.calls))
    ms["composed"].append(timed(composed, max(1, args.calls // 5)))

L.profile_enable(True)      # per-kernel events: a pass of its own (the brackets cost host time)
L.profile_reset()
reps = 5
for _ in range(reps):
    native()
torch.cuda.synchronize()
kern = {}
for name in ("blend_points", "track_flow_rows"):
    total, launches = L.profile_read(name)
    kern[name] = {"ms_per_call": total / reps, "launches_per_call": launches / reps}
L.profile_enable(False)

stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "rounds": len(v)}
rec = {"bench": "track_query", "build_id": L.build_id(), "device": torch.cuda.get_device_name(0),
       "gaussians": N, "W": W, "H": H, "target_frames": T, "queries": Q, "row_channels": 3 * T,
       "native_track_pixels": stat(ms["native"]), "composed_route": stat(ms["composed"]),
       "composed_over_native_median": float(np.median(ms["composed"]) / np.median(ms["native"])),
       "kernels": kern, "max_abs_track_difference_px": diff,
       "calls_per_window": {"native": args.calls, "composed": max(1, args.calls // 5)},
       "timing": "device events around a window of consecutive calls + synchronise, ms per call; windows of the two routes alternate in "
                 "one process after 2 warm-up calls of each; kernel times from the library's own per-kernel events, not a tracer"}
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
