"""Training a dynamic batch under per-frame and pinhole cameras (render_dynamic_sets(differentiable=True), the
Gaussian-side backward of include/splat_hip_views_grad.h) against the only differentiable route there was, at the project's
bench shape: 300k dynamic Gaussians, 854 x 480, the row rgb | depth | mask_attribute, 10 frames per batch, the reference's
orbit (views.orbit_cameras) -- orthographic, and the pinhole scene of make_scene(ortho=False) with the canonical intrinsics.

  batch       (a) render_dynamic_sets(extr [F,4,4], intr=, differentiable=True) and its backward: one batched forward under
              the frames' cameras, one tile backward, one Gaussian-side walk
  per_frame   (b) per frame dynamics.evaluate under autograd, a one-frame static FrameBatch.render_sets(extr_f, intr=...) and
              its backward
  one_camera  (c) the differentiable batch under ONE camera.  Orthographic: the path that was always differentiable (the
              CAM = 0 kernel), so (a) - (c) is the price of the camera per frame.  Pinhole: one camera through the same new
              kernel with both strides 0 (there is no older pinhole batch to compare with)

(a) and (b) must agree on every parameter gradient and the colours' (the rule of tests/test_gpu_parity.py::assert_grad at 5e-3:
the two routes may round a radius differently) before anything is timed; the tool fails on a disagreement after it has
written its record.  Forward + backward of one batch, legs alternating in one process, each timed with device events after a
warm-up of every leg; ms per frame = batch time / frames, median (min .. max) over the windows.  One JSON record (commit stamp
of tools/stamp.py, build id) goes to stdout and to --out.

    python tools/view_backward_bench.py [--windows 10] [--out profiles/view_backward.json]
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
from splatter_a_video_amd import views as V  # noqa: E402
from splatter_a_video_amd.dynamics import SEGMENT_MAJOR, FrameClock, evaluate, to_segment_major  # noqa: E402
from splatter_a_video_amd.frames import FrameBatch  # noqa: E402
from splatter_a_video_amd.renderer import OrthoEnhancedRenderer  # noqa: E402
from splatter_a_video_amd.synth import make_scene  # noqa: E402
from stamp import stamp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=10)
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--clip", type=int, default=50)
ap.add_argument("--frames-per-batch", type=int, default=10)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "view_backward.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("view_backward_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, T, F = args.gaussians, args.width, args.height, args.clip, args.frames_per_batch
dev = torch.device("cuda:0")
GEO = ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")
TRAIN = ("position", "pos_cubic_node", "rotation", "opacity", "scaling")
times = list(range(F))


def scene(ortho):
    sc = make_scene(N, W, H, F=T, seed=1234, ortho=ortho)
    clock = FrameClock(sc.F)
    par = TS.synthetic_video_params(sc, clock, dev)
    par["pos_cubic_node"] = to_segment_major(par["pos_cubic_node"], clock.interval_num)
    geo = {k: par[k].detach().clone().requires_grad_(k in TRAIN) for k in GEO}
    base = torch.tensor(sc.extr, device=dev)
    # the reference's orbit (radius 0.05) in front of the scene's own camera, about the middle of its depth range
    orbit = (V.orbit_cameras(T, radius=0.05, z_center=1.0 if ortho else 4.0, device=dev) @ base)[:F].contiguous()
    rgb = OrthoEnhancedRenderer.colors(par["shs"]).detach().clone().requires_grad_(True)
    mask = par["attrs"][:, :1].contiguous()
    g = torch.Generator(device="cpu").manual_seed(7)
    grads = [torch.randn(F, c, H, W, generator=g).to(dev) for c in (3, 1, 1)]
    return dict(clock=clock, geo=geo, orbit=orbit, intr=None if ortho else V.canonical_intrinsics(W, H, device=dev),
                nearest=0.01 if ortho else 0.2, rgb=rgb, grads=grads,
                sets=[dict(feature=rgb, bg=1.0, taps=True), dict(feature="depth", bg=1.0), dict(feature=mask, bg=0.0, detach_opacity=True)],
                fb=FrameBatch(F, N, W, H, 5, dev), one=FrameBatch(1, N, W, H, 5, dev))


def leaves(s):
    return [s["geo"][k] for k in TRAIN] + [s["rgb"]]


def clear(s):
    for t in leaves(s):
        t.grad = None


def batch(s):
    clear(s)
    res = s["fb"].render_dynamic_sets(s["clock"], times, s["orbit"], s["sets"], intr=s["intr"], nearest=s["nearest"],
                                      cubic_layout=SEGMENT_MAJOR, differentiable=True, **s["geo"])
    torch.autograd.backward(list(res[:3]), s["grads"])


def one_camera(s):
    clear(s)
    res = s["fb"].render_dynamic_sets(s["clock"], times, s["orbit"][0].contiguous(), s["sets"], intr=s["intr"], nearest=s["nearest"],
                                      cubic_layout=SEGMENT_MAJOR, differentiable=True, **s["geo"])
    torch.autograd.backward(list(res[:3]), s["grads"])


def per_frame(s):
    clear(s)
    for f, t in enumerate(times):
        pos, rot, opa, scl = evaluate(s["clock"], t, cubic_layout=SEGMENT_MAJOR, **s["geo"])
        res = s["one"].render_sets(pos, scl, rot, opa, s["sets"], None, s["orbit"][f].contiguous(), nearest=s["nearest"], intr=s["intr"])
        torch.autograd.backward(list(res[:3]), [g[f:f + 1] for g in s["grads"]])


def grads_of(s):
    return {k: t.grad.detach().double().cpu().numpy().reshape(-1) for k, t in zip(TRAIN + ("rgb",), leaves(s))}


def disagreement(a, b, tol=5e-3, atol_frac=1e-4):
    """tests/test_gpu_parity.py::assert_grad: (share of the elements outside tol |b| + atol_frac max|b|, worst error / max|b|)"""
    mx = max(float(np.abs(b).max()), 1e-30)
    err = np.abs(a - b)
    return float((err > tol * np.abs(b) + atol_frac * mx).mean()), float(err.max() / mx)


S = {"ortho": scene(True), "pinhole": scene(False)}
# ---- (a) and (b) agree on the gradients: measured before anything is timed, asserted once the record is written
agree = {}
for name, s in S.items():
    batch(s)
    torch.cuda.synchronize()
    s["fb"].check()
    ga = grads_of(s)
    per_frame(s)
    torch.cuda.synchronize()
    gb = grads_of(s)
    agree[name] = {k: dict(zip(("share_outside", "worst_over_max"), disagreement(ga[k], gb[k]))) for k in ga}
    del ga, gb
LEGS = {f"{leg.__name__}_{name}": (leg, s) for name, s in S.items() for leg in (batch, per_frame, one_camera)}


def window(name):
    leg, s = LEGS[name]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    leg(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / F


for name in LEGS:                      # one warm-up batch of every leg
    window(name)
ms = {name: [] for name in LEGS}
for _ in range(args.windows):
    for name in LEGS:
        ms[name].append(window(name))
stat = lambda v: {"median_ms_per_frame": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3),
                  "windows": len(v)}
med = lambda k: float(np.median(ms[k]))
rec = {"bench": "view_backward", **stamp(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "gaussians": N, "W": W, "H": H,
       "frames_per_batch": F, "row": "rgb 3 | depth 1 | mask_attribute 1", "what": "forward + backward of one batch",
       "batch_vs_per_frame_gradients": agree, "legs": {name: stat(v) for name, v in ms.items()}}
for name in S:
    rec[f"per_frame_over_batch_{name}"] = round(med(f"per_frame_{name}") / med(f"batch_{name}"), 3)
    rec[f"batch_minus_one_camera_ms_{name}"] = round(med(f"batch_{name}") - med(f"one_camera_{name}"), 3)
    rec[f"one_camera_spread_ms_{name}"] = round(float(np.max(ms[f"one_camera_{name}"]) - np.min(ms[f"one_camera_{name}"])), 3)
# the Gaussian-side kernel alone, from the library's own events (a pass of its own): "gauss_bwd_cam" = the new instantiations,
# "gauss_bwd" = the one-camera kernel
kern = {}
for name, s in S.items():
    kern[name] = {}
    for leg, event in ((batch, "gauss_bwd_cam"), (one_camera, "gauss_bwd_cam" if s["intr"] is not None else "gauss_bwd")):
        L.profile_reset()
        L.profile_enable(True)
        leg(s)
        torch.cuda.synchronize()
        L.profile_enable(False)
        t_ms, cnt = L.profile_read(event)
        kern[name][f"{leg.__name__}:{event}"] = {"us_per_frame": round(t_ms * 1e3 / F, 2), "launches": cnt}
    L.profile_reset()
rec["gauss_backward_kernel"] = kern
rec["timing"] = ("device events around forward + backward of one batch of frames, synchronise on both sides, ms per frame = batch time / "
                 "frames; the legs alternate in one process after the agreement check and one warm-up of each; median (min .. max) of the "
                 "windows; gradients are cleared inside the window; one run on a shared machine is a single sample")
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
bad = {f"{n}.{k}": v for n, d in agree.items() for k, v in d.items() if v["share_outside"] > 1e-4 or v["worst_over_max"] >= 3 * 5e-3}
assert not bad, f"the batch and the per-frame route disagree on gradients: {bad}"
