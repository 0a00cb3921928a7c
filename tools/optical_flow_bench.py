"""Dense optical flow of a clip (splatter_a_video_amd.flow, DESIGN "Dense optical flow") against the route that could be
composed before it, on the scene of the other tools: 300k dynamic Gaussians, 854 x 480, 25 pairs (t, t + 1) in batches of 5.

  render_flow  flow.render_flow: per batch one flow-attribute launch, one frame batch with the attribute as a per-frame tensor
  composed     per batch dynamics.positions_batch over the 2F frame times ([2F, P, 3]), the orthographic projection and its
               cull mask in torch (tests/torch_twin.py: project_point_ortho) for both times, the subtraction, then the same
               FrameBatch.render_dynamic_sets
  colours      flow.flow_to_image on the device against the reference's numpy colouring of the flow copied to the host
               (restated in tests/flow_ref.py)
  attribute    the attribute kernel alone (device events around 10 launches of 25 pairs), forward and backward
  train        render_flow(differentiable=True) forward + backward of one batch

The two routes must agree within the image rule scaled by the attribute's magnitude (compared before anything is timed).
One JSON record (commit stamp of tools/stamp.py, build id) goes to stdout and to --out: one sample on a shared machine.

    python tools/optical_flow_bench.py [--windows 5] [--out profiles/optical_flow.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from splatter_a_video_amd import _lib as L  # noqa: E402
from splatter_a_video_amd import flow as FL  # noqa: E402
from splatter_a_video_amd import train_step as TS  # noqa: E402
from splatter_a_video_amd.dynamics import SEGMENT_MAJOR, FrameClock, frame_table, positions_batch, to_segment_major  # noqa: E402
from splatter_a_video_amd.frames import FrameBatch  # noqa: E402
from splatter_a_video_amd.synth import make_scene  # noqa: E402
from stamp import stamp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--pairs", type=int, default=25)
ap.add_argument("--frames-per-batch", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optical_flow.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("optical_flow_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, T, FPB = args.gaussians, args.width, args.height, args.pairs, args.frames_per_batch
dev = torch.device("cuda:0")
GEO = ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")
sc = make_scene(N, W, H, F=T + 1, seed=1234, ortho=True)
clock = FrameClock(sc.F)
I = clock.interval_num
par = TS.synthetic_video_params(sc, clock, dev)
par["pos_cubic_node"] = to_segment_major(par["pos_cubic_node"], I)
model = {k: par[k].detach() for k in GEO}
extr = torch.tensor(sc.extr, device=dev)
t1, t2 = [float(t) for t in range(T)], [float(t + 1) for t in range(T)]
kw = dict(frames_per_batch=FPB, cubic_layout=SEGMENT_MAJOR)


def render_flow(stats=None):
    with torch.no_grad():
        return FL.render_flow(model, clock, t1, t2, extr, W, H, stats=stats, **kw)["flow"]


def _project(p, nearest=0.01, extent=1.3):
    """tests/torch_twin.py: project_point_ortho on [.., 3] positions, as a chain of torch element-wise launches"""
    t = p @ extr[:3, :3].T + extr[:3, 3]
    u, v, d = (t[..., 0] + 1.0) * W / 2 - 0.5, (t[..., 1] + 1.0) * H / 2 - 0.5, t[..., 2]
    cull = (d <= nearest) | (u < (1 - extent) * W * 0.5) | (u > (1 + extent) * W * 0.5) | (v < (1 - extent) * H * 0.5) | (v > (1 + extent) * H * 0.5)
    return torch.stack([u, v], -1) * (~cull)[..., None].to(p.dtype)


FB = FrameBatch(FPB, N, W, H, 2, dev, records=False)


@torch.no_grad()
def composed():
    out = torch.empty(T, 2, H, W, device=dev)
    for b0 in range(0, T, FPB):
        a, b = t1[b0:b0 + FPB], t2[b0:b0 + FPB]
        pos = positions_batch(clock, a + b, model["position"], model["pos_cubic_node"], SEGMENT_MAJOR)       # [2F, P, 3]
        uv = _project(pos)
        attr = (uv[FPB:] - uv[:FPB]).contiguous()
        while True:
            row = FB.render_dynamic_sets(clock, a, extr, [dict(feature=attr, bg=0.0, detach_opacity=True)], cubic_layout=SEGMENT_MAJOR,
                                         **model)[0]
            try:
                FB.check()
                break
            except L.SplatError:
                FB._grow(int(FB.pairs.max().item()))
        out[b0:b0 + FPB].copy_(row)
    return out


assert T % FPB == 0, "the composed route is written for whole batches"
st = {}
a, b = render_flow(st), composed()
torch.cuda.synchronize()
attr_max = float(FL.flow_attribute(clock, t1[:FPB], t2[:FPB], extr, W, H, position=model["position"], pos_cubic_node=model["pos_cubic_node"],
                                   cubic_layout=SEGMENT_MAJOR).abs().max())
outside = float(((a - b).abs() > 1e-5 * attr_max + 1e-4 * b.abs()).float().mean())
flow_maps = a


def host_colours():
    import flow_ref as FR
    return np.stack([FR.colours(f[None], scale="per_frame")[0][0] for f in flow_maps.cpu().numpy()])


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


tab1, tab2 = frame_table(clock, t1, dev), frame_table(clock, t2, dev)
cam1, _ = FL._pair_cameras(extr, None, None, None, T)
g_attr = torch.randn(T, N, 2, device=dev)
d_pos, d_cub = torch.zeros_like(model["position"]), torch.zeros_like(model["pos_cubic_node"])
attr_fwd = lambda: FL.flow_attribute_forward(tab1, tab2, model["position"], model["pos_cubic_node"], I, SEGMENT_MAJOR, cam1, None, W, H)
attr_bwd = lambda: FL.flow_attribute_backward(tab1, tab2, model["position"], model["pos_cubic_node"], I, SEGMENT_MAJOR, cam1, None, W, H,
                                              0.01, 1.3, False, g_attr, True, d_pos, d_cub)
live = dict(model, position=model["position"].clone().requires_grad_(True), pos_cubic_node=model["pos_cubic_node"].clone().requires_grad_(True))
g_img = torch.randn(FPB, 2, H, W, device=dev)


def train():
    out = FL.render_flow(live, clock, t1[:FPB], t2[:FPB], extr, W, H, differentiable=True, **kw)["flow"]
    out.backward(g_img)
    live["position"].grad = live["pos_cubic_node"].grad = None


LEGS = {"render_flow": lambda: timed(render_flow), "composed": lambda: timed(composed),
        "colours_device": lambda: timed(lambda: FL.flow_to_image(flow_maps), 10), "colours_host_numpy": lambda: wall(host_colours),
        "attribute_forward": lambda: timed(attr_fwd, 10), "attribute_backward": lambda: timed(attr_bwd, 10),
        "train_batch_forward_backward": lambda: timed(train)}
for leg in LEGS.values():
    leg()
ms = {k: [] for k in LEGS}
for _ in range(args.windows):
    for k, leg in LEGS.items():
        ms[k].append(leg())
stat = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4),
                  "windows": len(v)}
med = lambda k: float(np.median(ms[k]))
# bytes of the attribute kernel per (pair, Gaussian): two 48-byte spline records in, 8 bytes out (segment-major)
rec = {"bench": "optical_flow", **stamp(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "gaussians": N, "W": W, "H": H,
       "pairs": T, "frames_per_batch": FPB, "capacity": st["capacity"], "regrows": st["regrows"], "max_abs_attribute_px": round(attr_max, 3),
       "render_flow_vs_composed_share_outside_scaled_image_rule": outside, "legs": {k: stat(v) for k, v in ms.items()},
       "composed_over_render_flow": round(med("composed") / med("render_flow"), 3),
       "host_colours_over_device": round(med("colours_host_numpy") / med("colours_device"), 1),
       "attribute_forward_GBs_at_104_B_per_pair_gaussian": round(104.0 * T * N / (med("attribute_forward") * 1e-3) / 1e9, 1),
       "note": "one sample on a shared machine; legs alternate in one process, device events (host colours: wall clock incl. the copy)"}
text = json.dumps(rec, indent=1)
print(text)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
assert outside < 1e-3, f"render_flow and the composed route disagree on {outside:.2e} of the values"
