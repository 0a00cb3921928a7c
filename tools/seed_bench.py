"""The seeding stage (splatter_a_video_amd/seed.py) against what a user would run without it, three runs each on one GPU:

  1. median_filter_2d of one 854 x 480 frame, k = 11        vs  the torch-eager route (F.pad reflect + unfold + median)
  2. fit_cubic_nodes at N = 100 000 tracks, T = 100          vs  the reference's scipy loop on the host (one CubicSpline per
                                                                 point, src/dynamic_gaussian_with_base_point_cloud.py:69-78)
  3. lift_tracks at N = 10 000 tracks, T = 100, 854 x 480    vs  the same computation with F.grid_sample on the GPU

A GPU run is a window of --calls consecutive calls between two device events with a synchronise behind it (ms per call), after
two warm-up calls; the host loop is timed with the wall clock.  The native and the other route's outputs are compared.  One JSON
record, stamped with the commit and the library's build id, goes to --out.

    python tools/seed_bench.py [--calls 10] [--out profiles/seed_init.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from splatter_a_video_amd import _lib as L  # noqa: E402
from splatter_a_video_amd import seed  # noqa: E402
from splatter_a_video_amd.dynamics import FrameClock  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--spline-points", type=int, default=100000)
ap.add_argument("--lift-tracks", type=int, default=10000)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--commit", default=None, help="commit to stamp the record with (default: git describe of the tree)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_init.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("seed_bench needs the GPU: a timing taken anywhere else says nothing")
dev = torch.device("cuda:0")
W, H, T = 854, 480, args.frames
rng = np.random.default_rng(3)


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def gpu_runs(fn, calls):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


stat = lambda v: {"runs_ms": [float(x) for x in v], "median_ms": float(np.median(v)), "spread_ms": float(np.max(v) - np.min(v))}

# ---- 1. median
yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
disp = (0.6 + 0.3 * np.sin(xx / 90.0) * np.cos(yy / 70.0) + 0.05 * rng.normal(size=(H, W))).astype(np.float32)
frame = (1.0 / torch.clamp(torch.tensor(disp, device=dev), 1e-6, 1e6))[None, None]


def eager_median(x=frame, k=11):
    x = F.pad(x, (k // 2,) * 4, mode="reflect")
    x = x.unfold(2, k, 1).unfold(3, k, 1)
    return x.contiguous().view(x.size()[:4] + (-1,)).median(dim=-1)[0]


med_equal = bool(torch.equal(seed.median_filter_2d(frame, 11), eager_median()))
med_native = gpu_runs(lambda: seed.median_filter_2d(frame, 11), args.calls)
med_eager = gpu_runs(eager_median, max(1, args.calls // 5))

# ---- 2. spline
Ns = args.spline_points
walk = np.cumsum(0.02 * rng.normal(size=(Ns, T, 3)), axis=1).astype(np.float32)
tracks = torch.tensor(walk, device=dev)
clock = FrameClock(T)
fit_native = gpu_runs(lambda: seed.fit_cubic_nodes(tracks, clock), args.calls)
cubic = seed.fit_cubic_nodes(tracks, clock)[1].cpu().numpy().reshape(Ns, 4, clock.interval_num, 3)


def scipy_loop():
    from scipy.interpolate import CubicSpline
    idx = seed.knot_frames(clock, T)
    delta = (walk - walk[:, :1])[:, idx]
    return np.array([CubicSpline(clock.intervals, y).c for y in delta]).astype(np.float32)


fit_host = []
for _ in range(args.runs):
    t0 = time.perf_counter()
    ref = scipy_loop()
    fit_host.append((time.perf_counter() - t0) * 1e3)
fit_diff = float(np.abs(cubic - ref).max() / np.abs(ref).max())

# ---- 3. lifting
Nl = args.lift_tracks
depths = torch.tensor(rng.uniform(0.5, 2.0, size=(T, H, W)).astype(np.float32), device=dev)
masks = torch.tensor((rng.uniform(size=(T, H, W)) < 0.9).astype(np.float32), device=dev)
img = torch.tensor(rng.uniform(size=(H, W, 3)).astype(np.float32), device=dev)
t2 = np.empty((Nl, T, 4), np.float32)
t2[..., 0] = rng.uniform(-2, W + 1, size=(Nl, T))
t2[..., 1] = rng.uniform(-2, H + 1, size=(Nl, T))
t2[..., 2:] = rng.normal(-4.0, 2.5, size=(Nl, T, 2))
tracks_2d = torch.tensor(t2, device=dev)


def eager_lift(q=0):
    """get_tracks_3d_for_query_frame up to its `valid` selection, in torch on the GPU"""
    tr = tracks_2d.swapaxes(0, 1)
    xy, occ, dist = tr[..., :2], tr[..., 2], tr[..., 3]
    vis, conf = 1 - torch.sigmoid(occ), 1 - torch.sigmoid(dist)
    vv, vi = vis * conf > 0.5, (1 - vis) * conf > 0.5
    conf = conf * (vv | vi).float()
    grid = (xy / torch.tensor([W - 1.0, H - 1.0], device=dev) * 2 - 1.0)[:, None]
    d = F.grid_sample(depths[:, None], grid, align_corners=True, padding_mode="border")[:, 0, 0]
    wh = torch.tensor([W, H], device=dev)[None]
    t3 = torch.cat([(xy - wh / 2) / (wh / 2), d[..., None]], dim=-1)
    inm = F.grid_sample(masks[:, None], grid, align_corners=True)[:, 0, 0] == 1
    vv, vi, conf = vv & inm, vi & inm, conf * inm.float()
    counts = vv.sum(0), (conf > 0.5).sum(0)
    col = F.grid_sample(img[None].permute(0, 3, 1, 2), grid[q:q + 1], align_corners=True, padding_mode="border")[0, :, 0].T
    return t3.swapdims(0, 1), col, vv.swapdims(0, 1), vi.swapdims(0, 1), conf.swapdims(0, 1), counts


native_lift = lambda: seed._lift(tracks_2d, depths, masks, 0, img, False)
a, b = native_lift(), eager_lift()
lift_diff = float((a[0] - b[0]).abs().max())
lift_native = gpu_runs(native_lift, args.calls)
lift_eager = gpu_runs(eager_lift, max(1, args.calls // 2))

# ---- the kernels' own time: a pass of its own with the library's per-kernel events (the calls above include the host's share:
# tensor allocation and the ctypes call, which at these sizes is of the order of the kernels)
noise = torch.tensor(rng.normal(size=(1, 1, H, W)).astype(np.float32), device=dev)      # both signs: no shared leading key bits
L.profile_enable(True)
kern = {}
for name, fn in (("median_11", lambda: seed.median_filter_2d(frame, 11)), ("spline_fit", lambda: seed.fit_cubic_nodes(tracks, clock)),
                 ("lift_tracks", native_lift)):
    L.profile_reset()
    for _ in range(args.calls):
        fn()
    torch.cuda.synchronize()
    total, launches = L.profile_read(name)
    kern[name] = {"ms_per_launch": total / max(launches, 1), "launches": launches}
L.profile_reset()
for _ in range(args.calls):
    seed.median_filter_2d(noise, 11)
torch.cuda.synchronize()
total, launches = L.profile_read("median_11")
kern["median_11_signed_noise"] = {"ms_per_launch": total / max(launches, 1), "launches": launches}
L.profile_enable(False)

ratio = lambda other, mine: float(np.median(other) / np.median(mine))
rec = {"bench": "seed_init", "commit": commit(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0),
       "median_filter_2d": {"frame": [H, W], "kernel_size": 11, "native": stat(med_native), "torch_eager": stat(med_eager),
                            "eager_over_native": ratio(med_eager, med_native), "outputs_bit_equal": med_equal},
       "fit_cubic_nodes": {"points": Ns, "frames": T, "knots": int(clock.interval_num + 1), "native": stat(fit_native),
                           "scipy_host_loop": stat(fit_host), "host_over_native": ratio(fit_host, fit_native),
                           "max_abs_difference_over_max": fit_diff},
       "lift_tracks": {"tracks": Nl, "frames": T, "frame": [H, W], "native": stat(lift_native), "torch_grid_sample": stat(lift_eager),
                       "eager_over_native": ratio(lift_eager, lift_native), "max_abs_point_difference": lift_diff},
       "kernels": kern,
       "timing": f"{args.runs} runs per route; a GPU run = device events around a window of consecutive calls ({args.calls} native) + "
                 "synchronise, ms per call (host share included), after 2 warm-up calls; the scipy loop by the wall clock; spread = max - min "
                 "of the runs; kernels = the library's own per-kernel events around each launch, a pass of its own"}
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
