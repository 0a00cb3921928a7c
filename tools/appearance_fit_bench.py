"""Appearance editing (splatter_a_video_amd/edit.py) on the bench scene: 300k Gaussians at 854 x 480, the Gaussians
under a disc mask of about 10 % of the image selected, all their SH rows fitted to the frame rendered with other SH values on them.
ms per iteration of three routes:

  native_active   AppearanceFit, only the tiles whose list holds a selected Gaussian
  native_all      AppearanceFit(active_only=False): every tile in every iteration
  operators       the same fit through the existing operators: shs[selected] -> compute_sh -> gs.alpha_blending with only
                  ``feature`` requiring grad -> F.mse_loss -> backward -> torch.optim.Adam

The geometry is binned and sorted once for all three (the reference's loop repeats that per iteration as well; it is left out of
the operator route, which this favours).  A window is ``--steps`` consecutive iterations between two HIP events on the stream,
after warm-up iterations of every route; the routes' windows alternate in one process; median (min .. max) of the windows.  One
JSON line (with the commit stamp of tools/stamp.py and the build id) goes to stdout and to --out.

    python tools/appearance_fit_bench.py [--windows 5] [--steps 20] [--out profiles/appearance_fit.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from splatter_a_video_amd import _lib as L  # noqa: E402
from splatter_a_video_amd import gs  # noqa: E402
from splatter_a_video_amd.edit import AppearanceFit, select_gaussians  # noqa: E402
from splatter_a_video_amd.renderer import OrthoEnhancedRenderer  # noqa: E402
from splatter_a_video_amd.synth import make_scene  # noqa: E402
from stamp import stamp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--steps", type=int, default=20, help="iterations inside one timed window")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--mask-area", type=float, default=0.10)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "appearance_fit.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("appearance_fit_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, LR = args.gaussians, args.width, args.height, 0.0025
dev = torch.device("cuda:0")
t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
sc = make_scene(N, W, H, seed=1234)
shs, op = t(sc.shs), t(sc.opacity)
with torch.no_grad():
    uv, depth, conic, radius, tiles = gs.preprocess_ortho(t(sc.xyz), t(sc.scale), t(sc.rotate), t(sc.extr), W, H, nearest=0.01)
    idx, tr, _ = gs.sort_gaussian_capped(uv, depth, W, H, radius, None, conic, op)
    _, _, gs_idx = gs.alpha_blending_enhanced(uv, conic, op, OrthoEnhancedRenderer.colors(shs), idx, tr, 0.0, W, H, K=10)
    yy, xx = np.mgrid[0:H, 0:W]
    r2 = args.mask_area * W * H / np.pi
    mask = t(((xx - W / 2) ** 2 + (yy - H / 2) ** 2 < r2).astype(np.float32))
    sel = select_gaussians(gs_idx, mask, N)
    sel_idx = torch.nonzero(sel).reshape(-1)
    gen = torch.Generator(device=dev).manual_seed(7)
    edited = shs.clone()
    edited[sel] = shs[sel] + 0.3 * torch.randn(sel_idx.numel(), 16, 3, device=dev, generator=gen)
    target = gs.alpha_blending(uv, conic, op, OrthoEnhancedRenderer.colors(edited), idx, tr, 0.0, W, H).permute(1, 2, 0).contiguous()

fits = {"native_active": AppearanceFit(uv, depth, conic, radius, tiles, op, shs, sel, W, H, lr=LR),
        "native_all": AppearanceFit(uv, depth, conic, radius, tiles, op, shs, sel, W, H, lr=LR, active_only=False)}
history = torch.zeros(1 << 16, device=dev)
slot = {k: 0 for k in fits}
param = shs[sel_idx].clone().requires_grad_(True)
opt = torch.optim.Adam([param], lr=LR)
last = {}


def native(name):
    f = fits[name]
    with torch.no_grad():
        f._iteration(target, history, slot[name] % history.numel(), all_tiles=(slot[name] == 0))
    slot[name] += 1


def operators():
    full = shs.index_copy(0, sel_idx, param)
    img = gs.alpha_blending(uv, conic, op, OrthoEnhancedRenderer.colors(full), idx, tr, 0.0, W, H)
    loss = F.mse_loss(img.permute(1, 2, 0), target)
    opt.zero_grad()
    loss.backward()
    opt.step()
    last["operators"] = loss.detach()


LEGS = {"native_active": lambda: native("native_active"), "native_all": lambda: native("native_all"), "operators": operators}


def window(name, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        LEGS[name]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


for name in LEGS:
    window(name, args.warmup)
ms = {name: [] for name in LEGS}
for _ in range(args.windows):
    for name in LEGS:
        ms[name].append(window(name, args.steps))
stat = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4),
                  "windows": len(v)}
f_act = fits["native_active"]
rec = {"bench": "appearance_fit", **stamp(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "gaussians": N, "W": W,
       "H": H, "mask_area": args.mask_area, "selected": int(sel_idx.numel()), "tiles": f_act.T, "active_tiles": int(f_act.n_active),
       "pairs": int(f_act.M), "iterations_per_window": args.steps, "ms_per_iteration": {name: stat(v) for name, v in ms.items()}}
n_it = args.warmup + args.windows * args.steps
rec["loss_after_%d_iterations" % n_it] = {"native_active": float(history[slot["native_active"] - 1]), "operators": float(last["operators"])}
# per-kernel times of one more iteration of the two native routes from the library's own events (a pass of its own)
for name in fits:
    L.profile_reset()
    L.profile_enable(True)
    native(name)
    torch.cuda.synchronize()
    L.profile_enable(False)
    kern = {}
    for k in ("blend_fit_color", "tile_loss_sum", "pair_reduce", "adam"):
        t_ms, cnt = L.profile_read(k)
        if cnt:
            kern[k] = {"us": round(t_ms * 1e3, 1), "launches": cnt}
    rec["ms_per_iteration"][name]["kernels_us"] = kern
L.profile_reset()
med = lambda n: rec["ms_per_iteration"][n]["median_ms"]
rec["operators_over_native_all"] = round(med("operators") / med("native_all"), 3)
rec["operators_over_native_active"] = round(med("operators") / med("native_active"), 3)
rec["native_all_faster_than_operators"] = bool(med("native_all") < med("operators"))
rec["timing"] = ("HIP events on the stream around a window of consecutive iterations, ms per iteration; the routes' windows alternate "
                 "in one process after warm-up iterations of each; median (min .. max) of the windows; one run on a shared machine is "
                 "a single sample")
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
