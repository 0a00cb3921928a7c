"""Novel-view and stereo clips (splatter_a_video_amd.views, DESIGN "Novel views and stereo") against the routes the project
offered before them, on the scene of the other tools: 300k dynamic Gaussians, 854 x 480, a clip of 50 frames in batches of 10,
the reference renderer's row (rgb | depth | mask_attribute).  Two scenes: the orthographic one under the reference's orbit
(views.orbit_cameras about the video camera), and the pinhole scene of make_scene(ortho=False) under the same orbit in front of
its own camera with the canonical intrinsics.

  views       (a) render_views over the orbit: per batch one preprocess launch under the frames' cameras, one binning, one sort,
              one compositing pass
  per_frame   (b) the only route without a camera per frame: per frame dynamics.evaluate, then a one-frame static
              FrameBatch.render_sets(extr=extr_f, intr=...)
  one_camera  (c) render_views of the same clip under ONE camera (the single-camera kernel of the training path):
              (a) - (c) is the price of the camera per frame
  stereo      (d) render_stereo per stereo frame, against two_views: render_views of each eye (colours only) plus torch's
              clamp / einsum / cast; and the present kernel alone in GB/s (27 B per pixel with two eyes, 15 B with one)
              against what a float4 copy reaches on the MI355X (6.29 TB/s of the 8 TB/s peak)

(a) and (b) must agree: every set's image within IMG_ATOL + IMG_RTOL |ref| on all but 1e-3 of its values per frame (compared
before anything is timed; the tool fails on a disagreement after it has written its record).  Whole clips alternate in one
process, each timed with device events after a warm-up clip of every leg; ms per frame = clip time / frames, median (min .. max)
over the windows.  One JSON record (commit stamp of tools/stamp.py, build id) goes to stdout and to --out.

    python tools/novel_view_bench.py [--windows 10] [--out profiles/novel_views.json]
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

IMG_ATOL, IMG_RTOL = 1e-5, 1e-4          # the image rule of the GPU tests (tests/test_gpu_parity.py)
COPY_TBS = 6.29                          # a float4 copy on the MI355X (HBM3E peak: 8 TB/s)

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=10)
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--clip", type=int, default=50)
ap.add_argument("--frames-per-batch", type=int, default=10)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "novel_views.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("novel_view_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, T, FPB = args.gaussians, args.width, args.height, args.clip, args.frames_per_batch
dev = torch.device("cuda:0")
GEO = ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")
times = list(range(T))


def scene(ortho):
    sc = make_scene(N, W, H, F=T, seed=1234, ortho=ortho)
    clock = FrameClock(sc.F)
    par = TS.synthetic_video_params(sc, clock, dev)
    par["pos_cubic_node"] = to_segment_major(par["pos_cubic_node"], clock.interval_num)
    model = {k: par[k] for k in GEO}
    model["shs"] = par["shs"]
    model["mask_attribute"] = par["attrs"][:, :1].contiguous()
    base = torch.tensor(sc.extr, device=dev)
    # the reference's orbit (radius 0.05) in front of the scene's own camera, about the middle of its depth range
    orbit = (V.orbit_cameras(T, radius=0.05, z_center=1.0 if ortho else 4.0, device=dev) @ base).contiguous()
    eyes = (V.stereo_cameras(radius=0.05, at_z=2.5 if ortho else 4.0, device=dev) @ base).contiguous()
    intr = None if ortho else V.canonical_intrinsics(W, H, device=dev)
    nearest = 0.01 if ortho else 0.2
    rgb = OrthoEnhancedRenderer.colors(par["shs"]).detach()
    sets = [dict(feature=rgb, bg=1.0, taps=True), dict(feature="depth", bg=1.0),
            dict(feature=model["mask_attribute"], bg=0.0, detach_opacity=True)]
    return dict(clock=clock, model=model, geo={k: par[k] for k in GEO}, base=base, orbit=orbit, eyes=eyes, intr=intr, nearest=nearest,
                sets=sets, rgb=rgb, one=FrameBatch(1, N, W, H, 5, dev))


S = {"ortho": scene(True), "pinhole": scene(False)}
kw = lambda s: dict(frames_per_batch=FPB, cubic_layout=SEGMENT_MAJOR, nearest=s["nearest"])


def views(s, stats=None):
    return V.render_views(s["model"], s["clock"], times, s["orbit"], W, H, intr=s["intr"], stats=stats, **kw(s))


def one_camera(s):
    return V.render_views(s["model"], s["clock"], times, s["orbit"][0].contiguous(), W, H, intr=s["intr"], **kw(s))


@torch.no_grad()
def per_frame(s):
    outs = [torch.empty(T, w, H, W, device=dev) for w in (3, 1, 1)]
    for f, t in enumerate(times):
        pos, rot, opa, scl = evaluate(s["clock"], t, cubic_layout=SEGMENT_MAJOR, **s["geo"])
        res = s["one"].render_sets(pos, scl, rot, opa, s["sets"], None, s["orbit"][f].contiguous(), nearest=s["nearest"], intr=s["intr"])
        for o, r in zip(outs, res[:3]):
            o[f].copy_(r[0])
    return dict(zip(("rgb", "depth", "mask_attribute"), outs))


def stereo(s):
    return V.render_stereo(s["model"], s["clock"], times, W, H, cameras=s["eyes"], intr=s["intr"], **kw(s))


MIX = torch.tensor(V.ANAGLYPH["optimized"], device=dev)


def two_views(s):
    rgb = [dict(name="rgb", feature=s["rgb"], bg=1.0, taps=True)]
    l, r = (V.render_views(s["model"], s["clock"], times, e.contiguous(), W, H, intr=s["intr"], sets=rgb, **kw(s))["rgb"] for e in s["eyes"])
    cat = torch.cat([l.clamp(0, 1), r.clamp(0, 1)], dim=1)
    return (torch.einsum("tkhw,lk->thwl", cat, MIX) * 255).clamp(0, 255).to(torch.uint8)


# ---- (a) and (b) agree (the image rule): measured before anything is timed, asserted once the record is written
worst, pairs = {}, {}
for name, s in S.items():
    st = {}
    a, b = views(s, st), per_frame(s)
    torch.cuda.synchronize()
    worst[name] = 0.0
    for k in a:
        bad = ((a[k] - b[k]).abs() > (IMG_ATOL + IMG_RTOL * b[k].abs())).float().mean(dim=(1, 2, 3))
        worst[name] = max(worst[name], float(bad.max()))
    pairs[name] = dict(capacity=st["capacity"], regrows=st["regrows"], frame_batch_bytes=st["frame_batch_bytes"])
    del a, b
LEGS = {f"{leg.__name__}_{name}": (leg, s) for name, s in S.items() for leg in (views, per_frame, one_camera)}
LEGS.update({f"{leg.__name__}_ortho": (leg, S["ortho"]) for leg in (stereo, two_views)})


def window(name):
    leg, s = LEGS[name]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    leg(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / T


for name in LEGS:                      # one warm-up clip of every leg
    window(name)
ms = {name: [] for name in LEGS}
for _ in range(args.windows):
    for name in LEGS:
        ms[name].append(window(name))
stat = lambda v: {"median_ms_per_frame": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3),
                  "windows": len(v)}
med = lambda k: float(np.median(ms[k]))
rec = {"bench": "novel_views", **stamp(), "build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "gaussians": N, "W": W, "H": H,
       "clip_frames": T, "frames_per_batch": FPB, "row": "rgb 3 | depth 1 | mask_attribute 1", "batches": pairs,
       "views_vs_per_frame_worst_share_outside_image_rule": worst, "legs": {name: stat(v) for name, v in ms.items()}}
for name in S:
    rec[f"per_frame_over_views_{name}"] = round(med(f"per_frame_{name}") / med(f"views_{name}"), 3)
    rec[f"views_minus_one_camera_ms_{name}"] = round(med(f"views_{name}") - med(f"one_camera_{name}"), 3)
    rec[f"one_camera_spread_ms_{name}"] = round(float(np.max(ms[f"one_camera_{name}"]) - np.min(ms[f"one_camera_{name}"])), 3)
rec["two_views_over_stereo_ortho"] = round(med("two_views_ortho") / med("stereo_ortho"), 3)

# ---- the present kernel alone: T frames per launch, device events around `reps` launches
imgs = [torch.rand(T, 3, H, W, device=dev) * 1.4 - 0.2 for _ in range(2)]
present = {}
for key, fn, nbytes in (("anaglyph", lambda: V.anaglyph(imgs[0], imgs[1], "optimized"), 27), ("to_uint8", lambda: V.to_uint8(imgs[0]), 15)):
    fn()
    v = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        v.append(e0.elapsed_time(e1) / 10)
    gbs = [nbytes * H * W * T / (t * 1e-3) / 1e9 for t in v]
    present[key] = {"bytes_per_pixel": nbytes, "frames_per_launch": T, "median_us_per_launch": round(float(np.median(v)) * 1e3, 1),
                    "median_GBs": round(float(np.median(gbs)), 1), "min_GBs": round(float(np.min(gbs)), 1), "max_GBs": round(float(np.max(gbs)), 1),
                    "share_of_copy_bandwidth": round(float(np.median(gbs)) / (COPY_TBS * 1e3), 3)}
rec["present_kernel"] = present
rec["present_kernel"]["note"] = ("launch to launch on one stream, the output allocation included; algorithmic bytes (float planes in, bytes out) "
                                 f"over that time, against the {COPY_TBS} TB/s of a float4 copy")
# per-kernel times of one more orbit clip of each scene from the library's own events (a pass of its own)
kern = {}
for name, s in S.items():
    L.profile_reset()
    L.profile_enable(True)
    views(s)
    torch.cuda.synchronize()
    L.profile_enable(False)
    kern[name] = {}
    for k in ("frame_preprocess_fwd_cam", "bin_count", "bin_colscan", "bin_tilescan", "bin_scatter", "tile_sort", "blend_pack", "blend_fwd"):
        t_ms, cnt = L.profile_read(k)
        if cnt:
            kern[name][k] = {"us_per_frame": round(t_ms * 1e3 / T, 2), "launches": cnt}
    L.profile_reset()
    L.profile_enable(True)
    one_camera(s)
    torch.cuda.synchronize()
    L.profile_enable(False)
    t_ms, cnt = L.profile_read("frame_preprocess_fwd")
    kern[name]["one_camera:frame_preprocess_fwd*"] = {"us_per_frame": round(t_ms * 1e3 / T, 2), "launches": cnt}
    L.profile_reset()
rec["views_kernels"] = kern
rec["timing"] = ("device events around one whole clip, synchronise on both sides, ms per frame = clip time / frames; the legs' clips "
                 "alternate in one process after the agreement check and one warm-up clip of each; median (min .. max) of the windows; "
                 "every render_views / render_stereo call builds its FrameBatch and measures its pair capacity on its first batch (one "
                 "host synchronisation per batch reads the pair counts), the per_frame leg keeps one FrameBatch; one run on a shared "
                 "machine is a single sample")
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
assert all(v < 1e-3 for v in worst.values()), f"views and per_frame disagree: share of a frame's values outside the image rule {worst}"
