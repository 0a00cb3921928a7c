"""Layered clips seen from elsewhere (LayeredClip.render(extr=, intr=), DESIGN "Layered clips and feature lifting under
cameras") on the scene of tools/layer_edit_bench.py: 300k Gaussians, 854 x 480, a clip of 50 frames in batches of 10, a 30 %
foreground copied once at a delay of two frames, scaled by 0.6 and drifting (Q = 390k instances).

  orbit_ortho     (1) the layered clip under the reference's orbit (views.orbit_cameras, one orthographic camera per frame):
                  frame_preprocess_fwd_layer_cam_kernel<XF, 1>
  orbit_pinhole   (1) the same under a pinhole orbit two units in front of the scene (focal lengths 0.8 W / 0.8 H, nearest 0.2):
                  frame_preprocess_fwd_layer_cam_kernel<XF, 2>
  one_camera      (2) the same layered clip under ONE orthographic camera: the path of the parent commit
                  (frame_preprocess_fwd_layer_kernel); (1) - (2) is the price of the cameras
  same_camera_T   (2') the camera of (2) handed over as T equal per-frame cameras: the picture, lists and compositing of (2)
                  through the kernel of (1), so (2') - (2) is the price of the cameras alone ((1) renders another picture)
  per_frame_*     (3) the only route to (1) before this change: per frame dynamics.evaluate at both times, the transform in torch
                  (mask / mean / scale / cat) and a one-frame FrameBatch(1, Q).render_sets under that frame's camera
  bytes           (4) the clip's FrameBatch without the backward's pair-record buffer (records=False, what LayeredClip builds)
                  and with it, at the capacity the clip settled on

(1) and (3) must agree before anything is timed: every set's image within IMG_ATOL + IMG_RTOL |ref| on all but 1e-3 of its
values per frame.  Whole clips alternate in one process, each timed with device events after a warm-up clip of every leg; ms
per frame = clip time / frames, median (min .. max) over the windows.  The preprocess kernels' own times come from the library's
launch events in one more pass per leg.  One JSON record (commit stamp of tools/stamp.py, build id) goes to stdout and --out.

    python tools/layer_views_bench.py [--windows 10] [--out profiles/layer_views.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from splatter_a_video_amd import _lib as L  # noqa: E402
from splatter_a_video_amd import train_step as TS  # noqa: E402
from splatter_a_video_amd import views as V  # noqa: E402
from splatter_a_video_amd.dynamics import SEGMENT_MAJOR, FrameClock, evaluate, to_segment_major  # noqa: E402
from splatter_a_video_amd.frames import FrameBatch  # noqa: E402
from splatter_a_video_amd.layers import Layer, LayeredClip  # noqa: E402
from splatter_a_video_amd.renderer import OrthoEnhancedRenderer  # noqa: E402
from splatter_a_video_amd.synth import make_scene  # noqa: E402
from stamp import stamp  # noqa: E402

IMG_ATOL, IMG_RTOL = 1e-5, 1e-4          # the image rule of the GPU tests (tests/test_gpu_parity.py)

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=10)
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--clip", type=int, default=50)
ap.add_argument("--frames-per-batch", type=int, default=10)
ap.add_argument("--foreground", type=float, default=0.3)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "layer_views.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("layer_views_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, T, FPB = args.gaussians, args.width, args.height, args.clip, args.frames_per_batch
DELAY, SCALE, NEAREST_PINHOLE = 2, 0.6, 0.2
dev = torch.device("cuda:0")
sc = make_scene(N, W, H, F=T, seed=1234)
clock = FrameClock(sc.F)
par = TS.synthetic_video_params(sc, clock, dev)
par["pos_cubic_node"] = to_segment_major(par["pos_cubic_node"], clock.interval_num)
extr = torch.tensor(sc.extr, device=dev)
cam_xy = (sc.xyz @ sc.extr[:3, :3].T + sc.extr[:3, 3])[:, :2]
r2 = (cam_xy ** 2).sum(1)
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
layers = lambda: [Layer(), Layer(select=fg, times=ltimes, scale=SCALE, delta=delta)]

# the reference's orbit (radius 0.05) about the video camera; the pinhole orbit stands two units in front of the scene
orbit = (V.orbit_cameras(T, radius=0.05, z_center=1.0, device=dev) @ extr).contiguous()
phi = torch.linspace(0, 4 * math.pi, T)
back = torch.stack((0.05 * torch.cos(phi), 0.05 * torch.sin(phi), torch.full_like(phi, -2.0)), dim=1)
orbit_p = (V._world_to_camera(back, 0.5, dev) @ extr).contiguous()
intr = torch.tensor([0.8 * W, 0.8 * H, W / 2, H / 2], dtype=torch.float32, device=dev)

same_T = extr[None].repeat(T, 1, 1).contiguous()
CAMS = {"ortho": (orbit, None, 0.01), "pinhole": (orbit_p, intr, NEAREST_PINHOLE)}
clips = {k: LayeredClip(geo, clock, layers(), extr, W, H, sets_of(rgb, mask), frames_per_batch=FPB, cubic_layout=SEGMENT_MAJOR,
                        nearest=n_) for k, (_, _, n_) in CAMS.items()}
one = FrameBatch(1, Q, W, H, 5, dev)
rgb_q, mask_q = torch.cat([rgb, rgb[fg]]).contiguous(), torch.cat([mask, mask[fg]]).contiguous()
delta_dev = delta.to(dev)


@torch.no_grad()
def per_frame(kind):
    e_, i_, nearest = CAMS[kind]
    outs = [torch.empty(T, w, H, W, device=dev) for w in (3, 1, 1)]
    for f, (t, lt) in enumerate(zip(times, ltimes)):
        pos, rot, opa, scl = evaluate(clock, t, cubic_layout=SEGMENT_MAJOR, **geo)
        pos2, rot2, opa2, scl2 = evaluate(clock, lt, cubic_layout=SEGMENT_MAJOR, **geo)
        fg_pos = pos2[fg]
        mean = fg_pos.mean(dim=0, keepdim=True)
        fg_pos = (fg_pos - mean) * SCALE + mean
        fg_pos = fg_pos + delta_dev[f:f + 1]
        res = one.render_sets(torch.cat([pos, fg_pos]), torch.cat([scl, scl2[fg]]), torch.cat([rot, rot2[fg]]),
                              torch.cat([opa, opa2[fg]]), sets_of(rgb_q, mask_q), None, e_[f].contiguous(), nearest=nearest, intr=i_)
        for o, r in zip(outs, res[:3]):
            o[f].copy_(r[0])
    return outs


def orbit_clip(kind):
    e_, i_, _ = CAMS[kind]
    return clips[kind].render(times, extr=e_, intr=i_)


LEGS = {"orbit_ortho": lambda: orbit_clip("ortho"), "orbit_pinhole": lambda: orbit_clip("pinhole"),
        "one_camera": lambda: clips["ortho"].render(times),
        "same_camera_T": lambda: clips["ortho"].render(times, extr=same_T),
        "per_frame_ortho": lambda: per_frame("ortho"), "per_frame_pinhole": lambda: per_frame("pinhole")}

# ---- (1) and (3) agree (the image rule), before anything is timed; the pair counts say how much each leg composites
worst, pairs = {}, {}
for kind in CAMS:
    a, b = orbit_clip(kind), per_frame(kind)
    torch.cuda.synchronize()
    pairs["orbit_" + kind] = int(clips[kind].fb.check())
    worst[kind] = 0.0
    for x, y, name in zip(a, b, ("rgb", "depth", "mask_attribute")):
        bad = ((x - y).abs() > (IMG_ATOL + IMG_RTOL * y.abs())).float().mean(dim=(1, 2, 3))
        worst[kind] = max(worst[kind], float(bad.max()))
        assert float(bad.max()) < 1e-3, f"{kind} {name}: {float(bad.max()):.3e} of a frame's values outside the image rule"
    assert float((a[0].abs().amax(dim=(1, 2, 3))).min()) > 0.1, f"{kind}: an empty frame"
    del a, b
LEGS["one_camera"]()
torch.cuda.synchronize()
pairs["one_camera"] = int(clips["ortho"].fb.check())


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
med = lambda name: float(np.median(ms[name]))

# ---- the preprocess kernels' own times from the library's launch events (a pass of its own per leg)
kern = {}
for name in ("orbit_ortho", "orbit_pinhole", "one_camera", "same_camera_T"):
    L.profile_reset()
    L.profile_enable(True)
    LEGS[name]()
    torch.cuda.synchronize()
    L.profile_enable(False)
    t_cam, n_cam = L.profile_read("frame_preprocess_fwd_layer_cam")
    t_all, n_all = L.profile_read("frame_preprocess_fwd_layer")          # (a prefix: both kernels)
    t_cen, n_cen = L.profile_read("layer_centroid")
    kern[name] = {"layer_cam_kernel_us_per_frame": round(t_cam * 1e3 / T, 2), "layer_cam_launches": n_cam,
                  "layer_kernel_us_per_frame": round((t_all - t_cam) * 1e3 / T, 2), "layer_launches": n_all - n_cam,
                  "centroid_kernels_us_per_frame": round(t_cen * 1e3 / T, 2)}
L.profile_reset()

# ---- (4) the clip's frame batch without and with the backward's pair-record buffer
fb = clips["ortho"].fb
lean = fb.memory_bytes()
records = FPB * fb.capacity * fb.ncp * 4
full = FrameBatch(FPB, Q, W, H, 5, dev, capacity=fb.capacity)
full_bytes = full.memory_bytes()
assert full.pair_records.numel() * 4 == records and fb.pair_records is None and abs((full_bytes - records) - lean) <= 4
del full

rec = {"bench": "layer_views", **stamp(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "gaussians": N, "W": W, "H": H,
       "clip_frames": T, "frames_per_batch": FPB, "foreground": S, "Q": Q, "delay": DELAY, "scale": SCALE,
       "samples": {"windows_per_leg": args.windows, "runs": 1},
       "max_pairs_per_frame": pairs, "regrows": {k: c.regrows for k, c in clips.items()},
       "routes_worst_share_outside_image_rule": worst,
       "legs": {name: stat(v) for name, v in ms.items()},
       "orbit_ortho_minus_one_camera_ms_per_frame": round(med("orbit_ortho") - med("one_camera"), 3),
       "orbit_pinhole_minus_one_camera_ms_per_frame": round(med("orbit_pinhole") - med("one_camera"), 3),
       "same_camera_T_minus_one_camera_ms_per_frame": round(med("same_camera_T") - med("one_camera"), 3),
       "per_frame_over_orbit": {k: round(med("per_frame_" + k) / med("orbit_" + k), 3) for k in CAMS},
       "preprocess_kernels": kern,
       "frame_batch_bytes": {"without_records": lean, "with_records": full_bytes, "pair_record_bytes": records,
                             "capacity": fb.capacity, "record_stride_floats": fb.ncp},
       "timing": ("device events around one whole clip, synchronise on both sides, ms per frame = clip time / frames; the legs' clips "
                  "alternate in one process after the agreement check (one clip of each: the warm-up); median (min .. max) of the "
                  "windows; the pinhole orbit composites another picture than the orthographic legs (see max_pairs_per_frame), so "
                  "only its preprocess kernel time compares with theirs; one run on a shared machine is a single sample")}
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
