"""The camera gradients of a dynamic batch (render_dynamic_sets(camera_grad=True), the kernel of
include/splat_hip_camera_grad.h) at the shape of tools/view_backward_bench.py: 300k dynamic Gaussians, 854 x 480, the row rgb |
depth | mask_attribute, one batch of 10 frames, the reference's orbit -- orthographic cameras, and the pinhole scene of
make_scene(ortho=False) with the canonical intrinsics.

  constant     (a) render_dynamic_sets(extr [F,4,4], intr=, differentiable=True) and its backward: the path without camera leaves
  camera_grad  (b) the same with camera_grad=True, extr [F,4,4] (pinhole: and intr [4]) requiring grad: (b) - (a) is the price of
               the camera gradients (two launches more; three with the shared intr)
  per_operator (c) pinhole only: per frame dynamics.evaluate -> gs.project_point -> compute_cov3d -> ewa_project -> sort -> the three
               blends, the only route to a camera gradient there was (float atomics, one frame at a time)

Forward + backward, legs alternating in one process, each window = --reps batches between device events after a warm-up of every
leg; ms per frame, median (min .. max) over the windows.  Then, in passes of their own: the library's events "cam_grad",
"cam_grad_fold" and "gauss_bwd_cam" of leg (b), the kernel's achieved bytes/s against the record bytes it must touch (32 bytes +
the depth float of every record) and against the records' every byte, and a short pose-recovery curve (Adam on the
twists of views.pose_delta from a perturbed orbit; a demonstration, not an assertion).  One JSON record (commit stamp, build id)
goes to stdout and to --out.  Every figure is one sample on a shared machine.

    python tools/camera_grad_bench.py [--windows 10] [--out profiles/camera_grad.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dptr.gs as gs  # noqa: E402
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--clip", type=int, default=50)
ap.add_argument("--frames-per-batch", type=int, default=10)
ap.add_argument("--adam-steps", type=int, default=40)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "camera_grad.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("camera_grad_bench needs the GPU: a timing taken anywhere else says nothing")

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
    orbit = (V.orbit_cameras(T, radius=0.05, z_center=1.0 if ortho else 4.0, device=dev) @ base)[:F].contiguous()
    rgb = OrthoEnhancedRenderer.colors(par["shs"]).detach().clone().requires_grad_(True)
    mask = par["attrs"][:, :1].contiguous()
    g = torch.Generator(device="cpu").manual_seed(7)
    grads = [torch.randn(F, c, H, W, generator=g).to(dev) for c in (3, 1, 1)]
    intr = None if ortho else V.canonical_intrinsics(W, H, device=dev)
    return dict(clock=clock, geo=geo, orbit=orbit, intr=intr, nearest=0.01 if ortho else 0.2, rgb=rgb, mask=mask, grads=grads,
                extr_leaf=orbit.clone().requires_grad_(True), intr_leaf=None if ortho else intr.clone().requires_grad_(True),
                sets=[dict(feature=rgb, bg=1.0, taps=True), dict(feature="depth", bg=1.0), dict(feature=mask, bg=0.0, detach_opacity=True)],
                fb=FrameBatch(F, N, W, H, 5, dev))


def clear(s):
    for t in [s["geo"][k] for k in TRAIN] + [s["rgb"], s["extr_leaf"], s["intr_leaf"]]:
        if t is not None:
            t.grad = None


def constant(s):
    clear(s)
    res = s["fb"].render_dynamic_sets(s["clock"], times, s["orbit"], s["sets"], intr=s["intr"], nearest=s["nearest"],
                                      cubic_layout=SEGMENT_MAJOR, differentiable=True, **s["geo"])
    torch.autograd.backward(list(res[:3]), s["grads"])


def camera_grad(s):
    clear(s)
    res = s["fb"].render_dynamic_sets(s["clock"], times, s["extr_leaf"], s["sets"], intr=s["intr_leaf"], nearest=s["nearest"],
                                      cubic_layout=SEGMENT_MAJOR, differentiable=True, camera_grad=True, **s["geo"])
    torch.autograd.backward(list(res[:3]), s["grads"])


def per_operator(s):
    clear(s)
    for f, t in enumerate(times):
        pos, rot, opa, scl = evaluate(s["clock"], t, cubic_layout=SEGMENT_MAJOR, **s["geo"])
        e, k = s["extr_leaf"][f], s["intr_leaf"]
        uv, depth = gs.project_point(pos, k, e, W, H, s["nearest"], 1.3)
        vis = depth != 0
        cov = gs.compute_cov3d(scl, rot, vis)
        conic, radius, tiles = gs.ewa_project(pos, cov, k, e, uv, W, H, vis)
        idx, tr = gs.sort_gaussian(uv, depth, W, H, radius, tiles)
        ndc = torch.zeros_like(uv, requires_grad=True)
        imgs = [gs.alpha_blending(uv, conic, opa, s["rgb"], idx, tr, 1.0, W, H, ndc),
                gs.alpha_blending(uv, conic, opa, depth, idx, tr, 1.0, W, H, ndc),
                gs.alpha_blending(uv, conic, opa.detach(), s["mask"], idx, tr, 0.0, W, H, ndc)]
        torch.autograd.backward(imgs, [g[f] for g in s["grads"]])


S = {"ortho": scene(True), "pinhole": scene(False)}
LEGS = {f"{leg.__name__}_{name}": (leg, s) for name, s in S.items() for leg in (constant, camera_grad)}
LEGS["per_operator_pinhole"] = (per_operator, S["pinhole"])


def window(name):
    leg, s = LEGS[name]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.reps):
        leg(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (F * args.reps)


for name in LEGS:                      # one warm-up window of every leg
    window(name)
for s in S.values():
    s["fb"].check()
# the two routes to a pinhole camera gradient, side by side (per_operator sums with float atomics and makes its own decisions)
camera_grad(S["pinhole"])
ga = [S["pinhole"][k].grad.double().cpu().numpy() for k in ("extr_leaf", "intr_leaf")]
per_operator(S["pinhole"])
gb = [S["pinhole"][k].grad.double().cpu().numpy() for k in ("extr_leaf", "intr_leaf")]
agree = {k: round(float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)), 6) for k, a, b in zip(("extr", "intr"), ga, gb)}

ms = {name: [] for name in LEGS}
for _ in range(args.windows):
    for name in LEGS:
        ms[name].append(window(name))
stat = lambda v: {"median_ms_per_frame": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4),
                  "windows": len(v)}
med = lambda k: float(np.median(ms[k]))
rec = {"bench": "camera_grad", **stamp(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "gaussians": N, "W": W, "H": H,
       "frames_per_batch": F, "batches_per_window": args.reps, "row": "rgb 3 | depth 1 | mask_attribute 1",
       "what": "forward + backward of one batch; every figure is one sample on a shared machine",
       "legs": {name: stat(v) for name, v in ms.items()},
       "camera_grad_vs_per_operator_pinhole_worst_over_max": agree}
for name in S:
    a, b = f"constant_{name}", f"camera_grad_{name}"
    rec[f"camera_grad_minus_constant_us_per_frame_{name}"] = round((med(b) - med(a)) * 1e3, 2)
    rec[f"constant_spread_us_per_frame_{name}"] = round(float(np.max(ms[a]) - np.min(ms[a])) * 1e3, 2)
rec["per_operator_over_camera_grad_pinhole"] = round(med("per_operator_pinhole") / med("camera_grad_pinhole"), 3)

# ---- the kernels alone, from the library's own events (a pass of its own), and the bytes the new kernel must touch
kern = {}
stride = int(L.lib().splat_blend_sets_pair_stride(5))
for name, s in S.items():
    L.profile_reset()
    L.profile_enable(True)
    camera_grad(s)
    torch.cuda.synchronize()
    L.profile_enable(False)
    both, n_both = L.profile_read("cam_grad")
    fold, n_fold = L.profile_read("cam_grad_fold")
    walk, n_walk = L.profile_read("gauss_bwd_cam")
    L.profile_reset()
    pairs = int(s["fb"].pairs.sum().item())
    main_s = (both - fold) * 1e-3
    need = pairs * (32 + 4)                                                   # ux uy ga gb | gc .. and the depth float
    whole = pairs * stride * 4                                                # every byte of the records (what the walk reads)
    kern[name] = {"cam_grad_us_per_frame": round((both - fold) * 1e3 / F, 2), "cam_grad_launches": n_both - n_fold,
                  "cam_grad_fold_us_per_batch": round(fold * 1e3, 2), "cam_grad_fold_launches": n_fold,
                  "gauss_bwd_cam_us_per_frame": round(walk * 1e3 / F, 2), "gauss_bwd_cam_launches": n_walk,
                  "pair_records": pairs, "record_stride_floats": stride,
                  "needed_record_bytes": need, "achieved_GBps_needed_bytes": round(need / main_s / 1e9, 1),
                  "whole_record_bytes": whole, "achieved_GBps_whole_records": round(whole / main_s / 1e9, 1)}
rec["kernels"] = kern

# ---- pose recovery: Adam on the twists, from a perturbed orbit back to the orbit that rendered the target (a demonstration)
curve = {}
for name, s in S.items():
    with torch.no_grad():
        res = s["fb"].render_dynamic_sets(s["clock"], times, s["orbit"], s["sets"], intr=s["intr"], nearest=s["nearest"],
                                          cubic_layout=SEGMENT_MAJOR, differentiable=True, **s["geo"])
        target = res[0].clone()
    g = torch.Generator(device="cpu").manual_seed(11)
    pert = torch.cat([0.002 * torch.randn(F, 3, generator=g), 0.004 * torch.randn(F, 3, generator=g)], 1).to(dev)
    start = V.pose_delta(s["orbit"], pert)
    xi = torch.zeros(F, 6, device=dev, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=3e-4)
    geo = {k: v.detach() for k, v in s["geo"].items()}
    sets = [dict(feature=s["rgb"].detach(), bg=1.0, taps=True), s["sets"][1], s["sets"][2]]
    losses, errs = [], []
    for step in range(args.adam_steps + 1):
        opt.zero_grad()
        extr = V.pose_delta(start, xi)
        res = s["fb"].render_dynamic_sets(s["clock"], times, extr, sets, intr=s["intr"], nearest=s["nearest"],
                                          cubic_layout=SEGMENT_MAJOR, differentiable=True, camera_grad=True, **geo)
        loss = ((res[0] - target) ** 2).mean()
        losses.append(float(loss.detach()))
        errs.append(float((extr.detach() - s["orbit"]).norm(dim=(1, 2)).mean()))
        if step < args.adam_steps:
            loss.backward()
            opt.step()
    every = max(1, args.adam_steps // 10)
    curve[name] = {"lr": 3e-4, "perturbation": "N(0, 0.002) rad, N(0, 0.004) translation per frame",
                   "step": list(range(0, args.adam_steps + 1, every)), "mse": [round(v, 8) for v in losses[::every]],
                   "mean_pose_error_frobenius": [round(v, 6) for v in errs[::every]]}
rec["pose_recovery"] = curve
rec["timing"] = ("device events around --reps forward + backward batches, synchronise on both sides, ms per frame = window time / (frames "
                 "x batches); the legs alternate in one process after one warm-up window of each; median (min .. max) of the windows; "
                 "gradients are cleared inside the window; kernel times are the library's own events in a pass of their own; one run "
                 "on a shared machine is a single sample")
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
