"""Wide render attributes beside the composited row (FrameBatch.render_dynamic_sets(wide=...)) at bench.py's
training-frame workload: 300k Gaussians, 854 x 480, 25 frames of a 50-frame clip, K = 20, forward + backward with fixed random
gradient images.

  A          rgb | depth | track_gs + 16 attributes in the row (C = 23: the renderer's own plan), for context
  B32, B64   rgb | depth | track_gs in the row (C = 7) and wide= of 32 / 64 channels: one preprocess, one binning, one sort, one
             Gaussian-side walk
  C32, C64   what two batches give without wide=: the C = 7 row in one FrameBatch and 32 channels through render_dynamic in a
             second FrameBatch (twice over for 64), which preprocesses, bins, sorts and walks the Gaussians a second time (and
             blends with the live opacity: render_dynamic has no detached blend)

The legs' windows alternate in one process; a window is a host clock around consecutive forward + backward calls with a
synchronise on both sides (ms per call); median (min .. max) of the windows.  One JSON line (with the commit stamp of
tools/stamp.py and the build id) goes to stdout and to --out.

    python tools/wide_attr_bench.py [--windows 5] [--steps 4] [--out profiles/wide_attr.json]
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
from splatter_a_video_amd.dynamics import SEGMENT_MAJOR, FrameClock, frame_table, positions_batch_forward, to_segment_major  # noqa: E402
from splatter_a_video_amd.frames import FrameBatch  # noqa: E402
from splatter_a_video_amd.synth import make_scene  # noqa: E402
from stamp import stamp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--steps", type=int, default=4, help="forward + backward calls inside one timed window")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--frames", type=int, default=25)
ap.add_argument("--clip", type=int, default=50)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wide_attr.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("wide_attr_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, F, K = args.gaussians, args.width, args.height, args.frames, 20
dev = torch.device("cuda:0")
sc = make_scene(N, W, H, F=args.clip, seed=1234)
clock = FrameClock(sc.F)
I = clock.interval_num
par = TS.synthetic_video_params(sc, clock, dev, attrs=64)
par["pos_cubic_node"] = to_segment_major(par["pos_cubic_node"], I)
extr = torch.tensor(sc.extr, device=dev)
t1 = [i % sc.F for i in range(F)]
t2 = [int((17 * t + 11) % sc.F) for t in t1]
gen = torch.Generator(device=dev).manual_seed(7)
rgb = torch.rand(N, 3, device=dev, generator=gen)
pos2 = positions_batch_forward(frame_table(clock, t2, dev), par["position"], par["pos_cubic_node"], I, SEGMENT_MAJOR)      # track_gs [F, N, 3]
leaf = lambda t: t.detach().clone().requires_grad_(True)
lv = {k: leaf(par[k]) for k in ("pos_cubic_node", "rotation", "opacity", "scaling")}
lv["rgb"] = leaf(rgb)
for name, a, b in (("a16", 0, 16), ("a32", 0, 32), ("a32b", 32, 64), ("a64", 0, 64)):      # contiguous leaves: no slice copies in the legs
    lv[name] = leaf(par["attrs"][:, a:b].contiguous())
gimg = {c: torch.randn(F, c, H, W, device=dev, generator=gen) for c in (3, 1, 19, 32, 64)}
geo = dict(position=par["position"], pos_cubic_node=lv["pos_cubic_node"], rotation=lv["rotation"], rot_poly_feat=par["rot_poly_feat"],
           rot_fourier_feat=par["rot_fourier_feat"], opacity=lv["opacity"], scaling=lv["scaling"], cubic_layout=SEGMENT_MAJOR)
batches = {"A": FrameBatch(F, N, W, H, 23, dev), "B32": FrameBatch(F, N, W, H, 7, dev), "B64": FrameBatch(F, N, W, H, 7, dev),
           "C_row": FrameBatch(F, N, W, H, 7, dev), "C_wide": FrameBatch(F, N, W, H, 32, dev)}
row7 = lambda: [dict(feature=lv["rgb"], bg=0.0, taps=True), dict(feature="depth", bg=1.0),
                dict(feature=[pos2], bg=0.0, detach_opacity=True)]


def clear():
    for v in lv.values():
        v.grad = None


def leg_A():
    sets = row7()
    sets[2] = dict(feature=[pos2, lv["a16"]], bg=0.0, detach_opacity=True)
    out = batches["A"].render_dynamic_sets(clock, t1, extr, sets, K=K, **geo)
    torch.autograd.backward(list(out[:3]), [gimg[3], gimg[1], gimg[19]])


def leg_B(c):
    out = batches[f"B{c}"].render_dynamic_sets(clock, t1, extr, row7(), K=K,
                                               wide=dict(feature=lv[f"a{c}"], bg=0.0, detach_opacity=True), **geo)
    torch.autograd.backward(list(out[:4]), [gimg[3], gimg[1], gimg[19][:, :3].contiguous(), gimg[c]])


def leg_C(c):
    out = batches["C_row"].render_dynamic_sets(clock, t1, extr, row7(), K=K, **geo)
    torch.autograd.backward(list(out[:3]), [gimg[3], gimg[1], gimg[19][:, :3].contiguous()])
    for name in (("a32",) if c == 32 else ("a32", "a32b")):      # one forward at a time per batch: a half's backward before the next forward
        img = batches["C_wide"].render_dynamic(clock, t1, extr, lv[name], bg=0.0, **geo)
        img.backward(gimg[32])


LEGS = {"A": leg_A, "B32": lambda: leg_B(32), "B64": lambda: leg_B(64), "C32": lambda: leg_C(32), "C64": lambda: leg_C(64)}


def window(name, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        clear()
        LEGS[name]()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


for name in LEGS:
    window(name, args.warmup)
pairs = {k: int(b.check()) for k, b in batches.items()}
ms = {name: [] for name in LEGS}
for _ in range(args.windows):
    for name in LEGS:
        ms[name].append(window(name, args.steps))
stat = lambda v: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3),
                  "windows": len(v)}
rec = {"bench": "wide_attr", **stamp(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "gaussians": N, "W": W, "H": H,
       "frames": F, "K": K, "calls_per_window": args.steps, "max_pairs_per_frame": pairs,
       "legs": {name: stat(v) for name, v in ms.items()}}
# per-kernel times of one more call of the wide legs from the library's own events (a pass of its own)
for name in ("B32", "B64"):
    L.profile_reset()
    L.profile_enable(True)
    clear()
    LEGS[name]()
    torch.cuda.synchronize()
    L.profile_enable(False)
    kern = {}
    for k in ("blend_fwd", "blend_pack", "blend_bwd", "wide_fold", "gauss_bwd"):
        t_ms, cnt = L.profile_read(k)
        if cnt:
            kern[k] = {"us_per_call": round(t_ms * 1e3, 1), "launches": cnt}
    rec["legs"][name]["kernels_us_per_call"] = kern
L.profile_reset()
med = lambda n: rec["legs"][n]["median_ms"]
spread = lambda n: rec["legs"][n]["max_ms"] - rec["legs"][n]["min_ms"]
for c in (32, 64):
    gain = med(f"C{c}") - med(f"B{c}")
    rec[f"two_batches_minus_wide_{c}_ms"] = round(gain, 3)
    rec[f"wide_{c}_faster_by_more_than_either_spread"] = bool(gain > max(spread(f"B{c}"), spread(f"C{c}")))
rec["timing"] = ("host clock around a window of consecutive forward + backward calls, synchronise on both sides, ms per call; the legs' "
                 "windows alternate in one process after warm-up calls of each; median (min .. max) of the windows; one run on a "
                 "shared machine is a single sample")
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
