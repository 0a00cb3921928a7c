"""Layer editing (splatter_a_video_amd.layers, DESIGN "Layer editing") against the frame-by-frame composition the project
offered before it, on the scene of the other tools: 300k Gaussians, 854 x 480, a clip of 50 frames, a 30 % foreground (the
Gaussians nearest the image centre) copied once at a delay of two frames, scaled by 0.6 and drifting.

  layered    LayeredClip([whole model, transformed foreground copy]).render(times): per batch of frames one preprocess launch per
             layer (+ two centroid launches), one binning, one sort, one compositing pass
  per_frame  the reference's route (src/trainer_fragGS.py:1344-1405) from the existing operators, frame by frame:
             dynamics.evaluate at both times, torch mask / mean / scale / cat, FrameBatch(1, Q).render_sets (the time-invariant
             colour and mask rows are concatenated once, outside the timed loop)

Before anything is timed the two routes must agree: every set's image within IMG_ATOL + IMG_RTOL |ref| on all but 1e-3 of its
values per frame.  Then whole clips alternate in one process, each timed with device events after a warm-up clip of each route;
ms per frame = clip time / frames, median (min .. max) over the windows.  One JSON record (commit stamp of tools/stamp.py,
build id) goes to stdout and to --out.

    python tools/layer_edit_bench.py [--windows 5] [--out profiles/layer_edit.json]
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
from splatter_a_video_amd.dynamics import SEGMENT_MAJOR, FrameClock, evaluate, to_segment_major  # noqa: E402
from splatter_a_video_amd.frames import FrameBatch  # noqa: E402
from splatter_a_video_amd.layers import Layer, LayeredClip  # noqa: E402
from splatter_a_video_amd.renderer import OrthoEnhancedRenderer  # noqa: E402
from splatter_a_video_amd.synth import make_scene  # noqa: E402
from stamp import stamp  # noqa: E402

IMG_ATOL, IMG_RTOL = 1e-5, 1e-4          # the image rule of the GPU tests (tests/test_gpu_parity.py)

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--clip", type=int, default=50)
ap.add_argument("--frames-per-batch", type=int, default=10)
ap.add_argument("--foreground", type=float, default=0.3)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "layer_edit.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("layer_edit_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, T = args.gaussians, args.width, args.height, args.clip
DELAY, SCALE = 2, 0.6
dev = torch.device("cuda:0")
sc = make_scene(N, W, H, F=T, seed=1234)
clock = FrameClock(sc.F)
I = clock.interval_num
par = TS.synthetic_video_params(sc, clock, dev)
par["pos_cubic_node"] = to_segment_major(par["pos_cubic_node"], I)
extr = torch.tensor(sc.extr, device=dev)
cam = (sc.xyz @ sc.extr[:3, :3].T + sc.extr[:3, 3])[:, :2]
r2 = (cam ** 2).sum(1)
fg = torch.tensor(r2 < np.quantile(r2, args.foreground), device=dev)
S = int(fg.sum())
Q = N + S
mask = torch.where(fg, 0.9, 0.1).float()[:, None].contiguous()
rgb = OrthoEnhancedRenderer.colors(par["shs"]).detach()
times = list(range(T))
ltimes = [max(0, t - DELAY) for t in times]
delta = (torch.tensor([[0.25, -0.15, -0.2]]) + torch.tensor([[-0.002, 0.001, 0.0]]) * torch.tensor(ltimes, dtype=torch.float32)[:, None])
geo = {k: par[k] for k in ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")}
sets_of = lambda c, m: [dict(feature=c, bg=0.0, taps=True), dict(feature="depth", bg=1.0), dict(feature=m, bg=0.0, detach_opacity=True)]

clip = LayeredClip(geo, clock, [Layer(), Layer(select=fg, times=ltimes, scale=SCALE, delta=delta)], extr, W, H, sets_of(rgb, mask),
                   frames_per_batch=args.frames_per_batch, cubic_layout=SEGMENT_MAJOR)
one = FrameBatch(1, Q, W, H, 5, dev)
rgb_q, mask_q = torch.cat([rgb, rgb[fg]]).contiguous(), torch.cat([mask, mask[fg]]).contiguous()
delta_dev = delta.to(dev)


@torch.no_grad()
def per_frame():
    outs = [torch.empty(T, w, H, W, device=dev) for w in (3, 1, 1)]
    for f, (t, lt) in enumerate(zip(times, ltimes)):
        pos, rot, opa, scl = evaluate(clock, t, cubic_layout=SEGMENT_MAJOR, **geo)
        pos2, rot2, opa2, scl2 = evaluate(clock, lt, cubic_layout=SEGMENT_MAJOR, **geo)
        fg_pos = pos2[fg]
        mean = fg_pos.mean(dim=0, keepdim=True)
        fg_pos = (fg_pos - mean) * SCALE + mean
        fg_pos = fg_pos + delta_dev[f:f + 1]
        res = one.render_sets(torch.cat([pos, fg_pos]), torch.cat([scl, scl2[fg]]), torch.cat([rot, rot2[fg]]),
                              torch.cat([opa, opa2[fg]]), sets_of(rgb_q, mask_q), None, extr)
        for o, r in zip(outs, res[:3]):
            o[f].copy_(r[0])
    return outs


def layered():
    return clip.render(times)


# ---- the two routes agree (the image rule), before anything is timed
a, b = layered(), per_frame()
torch.cuda.synchronize()
worst = 0.0
for x, y, name in zip(a, b, ("rgb", "depth", "mask_attribute")):
    bad = ((x - y).abs() > (IMG_ATOL + IMG_RTOL * y.abs())).float().mean(dim=(1, 2, 3))
    worst = max(worst, float(bad.max()))
    assert float(bad.max()) < 1e-3, f"{name}: {float(bad.max()):.3e} of a frame's values outside the image rule"
del a, b
LEGS = {"layered": layered, "per_frame": per_frame}


def window(name):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    LEGS[name]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / T


ms = {name: [] for name in LEGS}
for _ in range(args.windows):
    for name in LEGS:
        ms[name].append(window(name))
stat = lambda v: {"median_ms_per_frame": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3),
                  "windows": len(v)}
rec = {"bench": "layer_edit", **stamp(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "gaussians": N, "W": W, "H": H,
       "clip_frames": T, "frames_per_batch": args.frames_per_batch, "foreground": S, "Q": Q, "delay": DELAY, "scale": SCALE,
       "max_pairs_per_frame": int(clip.fb.check()), "regrows": clip.regrows, "frame_batch_bytes": clip.fb.memory_bytes(),
       "pair_record_bytes": 0 if clip.fb.pair_records is None else int(clip.fb.pair_records.numel() * 4), "routes_worst_share_outside_image_rule": worst,
       "legs": {name: stat(v) for name, v in ms.items()}}
rec["per_frame_over_layered"] = round(rec["legs"]["per_frame"]["median_ms_per_frame"] / rec["legs"]["layered"]["median_ms_per_frame"], 3)
# per-kernel times of one more layered clip from the library's own events (a pass of its own)
L.profile_reset()
L.profile_enable(True)
layered()
torch.cuda.synchronize()
L.profile_enable(False)
kern = {}
for k in ("layer_centroid_partial", "layer_centroid_final", "frame_preprocess_fwd_layer", "bin_count", "bin_colscan", "bin_tilescan",
          "bin_scatter", "tile_sort", "blend_pack", "blend_fwd"):
    t_ms, cnt = L.profile_read(k)
    if cnt:
        kern[k] = {"us_per_frame": round(t_ms * 1e3 / T, 2), "launches": cnt}
L.profile_reset()
rec["layered_kernels"] = kern
rec["timing"] = ("device events around one whole clip, synchronise on both sides, ms per frame = clip time / frames; the two routes' "
                 "clips alternate in one process after the agreement check (one clip of each: the warm-up); median (min .. max) of "
                 "the windows; one run on a shared machine is a single sample")
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
