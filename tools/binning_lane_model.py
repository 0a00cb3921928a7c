#!/usr/bin/env python
"""CPU model of the tile loops of bin_count / bin_scatter (csrc/binning.hip): how many trips a wave runs when one lane takes one
Gaussian and loops over the tiles of its rectangle, for three visiting orders of a workgroup's chunk:
    stored   thread t takes beg + t + 256 k and walks whatever rectangle it meets (the kernels before the area order);
    area     the chunk walked by exact rectangle area, largest first (the best any order inside the chunk can do);
    classes  a counting sort of the chunk by area class, Gaussians without tiles left out (tried first, not kept: DESIGN 4ae);
    built    what the kernels do ("area order", csrc/binning.hip): in stored order a lane walks a rectangle of at most
             BIN_INLINE_AREA tiles and defers a larger one to a list, which the workgroup walks afterwards, rectangles of at least
             BIN_BIG_AREA tiles first.
A wave runs as many trips as the largest rectangle among its 64 Gaussians; lane utilisation = tiles / (64 * trips).
Needs no GPU: geometry from the C oracle, Gaussians in the Morton order the bench keeps (densify.spatial_order restated).
    python tools/binning_lane_model.py [--gaussians N] [--out profiles/binning_area_order_model.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import binning_ref as R  # noqa: E402  (rect, and the constants of csrc/binning.hip)

WAVE = 64
BIN_SEG = 2048
BIN_INLINE_AREA = 4        # the constants of csrc/binning.hip ("area order"); tests/test_binning_lane_model_cpu.py parses the source
BIN_BIG_AREA = 10
# lower bounds of the area classes of the counting sort that was tried first, largest first; the last class holds the Gaussians
# without tiles
CLASS_LOWER = [32, 17, 13, 10, 7, 5, 3, 2, 1, 0]


def area_class(area):
    """class index of every area: 0 = the largest rectangles"""
    return len(CLASS_LOWER) - np.searchsorted(np.asarray(CLASS_LOWER[::-1]), np.asarray(area), side="right")   # bounds above the area


def chunks(P: int, chunk: int):
    return [(b, min(P, b + chunk)) for b in range(0, P, chunk)]


# An order is a list of (local indices, mask) per pass over the chunk: thread t of the workgroup takes entry t + 256 k of the list
# and walks its rectangle where the mask is set (a lane whose mask is clear idles in that pass).
def order_stored(area, beg, end, seg=BIN_SEG):
    n = end - beg
    return [(np.arange(n), np.ones(n, bool))]


def order_area(area, beg, end, seg=BIN_SEG):
    a = area[beg:end]
    o = np.argsort(-a, kind="stable")
    o = o[a[o] > 0]
    return [(o, np.ones(o.size, bool))]


def order_classes(area, beg, end, seg=BIN_SEG):
    """the counting sort by area class (classes descending, index order inside a class), per segment, cut at the first Gaussian
    without tiles"""
    out = []
    for s in range(beg, end, seg):
        a = area[s:min(end, s + seg)]
        c = area_class(a)
        o = np.argsort(c, kind="stable")
        o = (s - beg) + o[c[o] < len(CLASS_LOWER) - 1]
        out.append((o, np.ones(o.size, bool)))
    return out


def order_built(area, beg, end, seg=BIN_SEG):
    """what the kernels do, per segment: a pass in stored order that walks the rectangles of at most BIN_INLINE_AREA tiles, then
    the deferred list, rectangles of at least BIN_BIG_AREA tiles first (index order inside both parts -- the kernels leave that to
    the race of the waves)"""
    out = []
    for s in range(beg, end, seg):
        a = area[s:min(end, s + seg)]
        idx = (s - beg) + np.arange(a.size)
        out.append((idx, a <= BIN_INLINE_AREA))
        d = np.concatenate([idx[a >= BIN_BIG_AREA], idx[(a > BIN_INLINE_AREA) & (a < BIN_BIG_AREA)]])
        out.append((d, np.ones(d.size, bool)))
    return out


def visits(area, beg, end, seg=BIN_SEG):
    """local indices in the order in which the built kernels walk the rectangles of a chunk (Gaussians without tiles: where the
    stored-order pass meets them)"""
    return np.concatenate([li[m] for li, m in order_built(area, beg, end, seg)] or [np.zeros(0, np.int64)])


def wave_trips(area, beg, passes, block=R.BIN_BLOCK):
    """trips summed over the waves: a wave runs max(area) trips over its 64 lanes"""
    trips = 0
    for li, mask in passes:
        a = np.where(mask, area[beg + li], 0)
        pad = (-a.size) % WAVE
        trips += int(np.concatenate([a, np.zeros(pad, a.dtype)]).reshape(-1, WAVE).max(axis=1).sum()) if a.size else 0
    return trips


ORDERS = (("stored", order_stored), ("area", order_area), ("classes", order_classes), ("built", order_built))


def model(area, chunk: int):
    P = area.size
    res = {}
    tiles = int(area.sum())
    groups = -(-P // WAVE)
    for name, fn in ORDERS:
        trips = sum(wave_trips(area, beg, fn(area, beg, end)) for beg, end in chunks(P, chunk))
        res[name] = {"trips_per_64_gaussians": round(trips / groups, 3), "lane_utilisation": round(tiles / (WAVE * max(trips, 1)), 4)}
    res["stored_over_built"] = round(res["stored"]["trips_per_64_gaussians"] / max(res["built"]["trips_per_64_gaussians"], 1e-9), 3)
    res["deferred_fraction"] = round(float((area > BIN_INLINE_AREA).mean()), 4)
    return res


def bench_areas(N, W, H, frames, seed=1234):
    import oracle
    from splatter_a_video_amd.synth import make_scene
    sc = make_scene(N, W, H, seed=seed)
    ext, intr = sc.extr, sc.intr

    def project(f):
        xyz = sc.positions(f)
        uv, _ = oracle.project_point_ortho_forward(xyz, ext, W, H, nearest=0.01)
        cov = oracle.compute_cov3d_forward(sc.scale, sc.rotate)
        _, radius, _ = oracle.ewa_project_forward(xyz, cov, intr, ext, uv, W, H, visible=None, ortho=True)
        return uv, radius

    uv0, _ = project(0)
    order = morton_order(uv0, W, H)
    out = []
    for f in frames:
        uv, radius = project(f)
        x0, y0, x1, y1 = R.rect(uv[order], radius[order], W, H)
        out.append(((x1 - x0) * (y1 - y0)).astype(np.int64))
    return out


def morton_order(uv, W, H):
    """densify.spatial_order (csrc/densify.hip: morton_keys_kernel) in numpy"""
    def spread(v):
        v = v.astype(np.uint32)
        v = (v | (v << 8)) & 0x00FF00FF
        v = (v | (v << 4)) & 0x0F0F0F0F
        v = (v | (v << 2)) & 0x33333333
        return (v | (v << 1)) & 0x55555555
    f32 = np.float32
    fx = np.clip(np.nan_to_num(uv[:, 0].astype(f32) * f32(32768.0 / W)), 0, 32767).astype(np.uint32)
    fy = np.clip(np.nan_to_num(uv[:, 1].astype(f32) * f32(32768.0 / H)), 0, 32767).astype(np.uint32)
    return np.argsort((spread(fx) | (spread(fy) << 1)).astype(np.int64), kind="stable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--width", type=int, default=854)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--frames", type=int, nargs="+", default=[0, 12])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binning_area_order_model.json"))
    a = ap.parse_args()
    P = a.gaussians
    plans = {"batch": R.plan(P, a.width, a.height, R.BIN_BATCH_FRAMES)["chunk"], "single_frame": R.plan(P, a.width, a.height, 1)["chunk"]}
    rec = {"source": "tools/binning_lane_model.py: CPU model, no GPU run", "scene": f"{P}x{a.width}x{a.height}, Morton order of frame 0",
           "inline_area": BIN_INLINE_AREA, "big_area": BIN_BIG_AREA, "class_lower_bounds_of_the_sort_tried": CLASS_LOWER, "segment": BIN_SEG, "chunk": plans, "frames": {}}
    for f, area in zip(a.frames, bench_areas(P, a.width, a.height, a.frames)):
        vals, cnt = np.unique(area, return_counts=True)
        rec["frames"][str(f)] = {"tiles": int(area.sum()), "tiles_per_gaussian": round(float(area.mean()), 3),
                                 "area_histogram": {int(v): int(c) for v, c in zip(vals, cnt)},
                                 **{k: model(area, c) for k, c in plans.items()}}
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps({f: {k: v for k, v in r.items() if k != "area_histogram"} for f, r in rec["frames"].items()}, indent=1))


if __name__ == "__main__":
    main()
