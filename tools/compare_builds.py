#!/usr/bin/env python3
"""Bit comparison of two builds of libsplat_hip.so on the frame-batch compositing paths.

The frame-batch paths use no float atomics and are bit-reproducible (tests/test_gpu_determinism.py), so a change that keeps
the arithmetic must reproduce another build bit for bit.  The driver never opens the GPU: it starts one fresh child process
per library (selected with SPLAT_LIB_PATH, same ABI), each child renders seeded scenes forward and backward and writes the
SHA-256 digest of every output; the driver compares the digests and writes the record.

    python tools/compare_builds.py --a path/to/libsplat_hip.so --b splatter_a_video_amd/libsplat_hip.so --out record.json

Outputs digested per case: images, final_T, ncontrib, the forward's cull words (the part of every tile's list that the
forward wrote; the rest of the buffer is uninitialised memory and masked), gs_idx
(three-set plans), every parameter gradient, taps and abs taps, the loss-fused per-tile sums.  Cases: narrow C = 1, 3 with
and without abs taps; wide C = 16, 19, 24, 32; the renderer's 3|1|19 plan on the forward's records and with sets_std = 0; the
3|1|4 and 3|1|8 plans; the loss-fused entry -- each on a scene of 250 x 187 pixels (ragged right and bottom tiles), 20000
Gaussians, F = 2, whose longest tile list must exceed two super-batches of the largest super-batch among the kernels (so that
staging, the prefetch's carry-over and the list build run more than once), and on a scene of 50 Gaussians (most tiles take
the empty-tile exit and the zero-record path).

The `points` family (--family points; csrc/query.hip): the sparse compositing at query points.  The forward entries and the ordered
backward entries use no float atomic; the atomic backward entries are digested on one-writer inputs only (a single integer query
pixel per frame on the scene's densest pixel, a per-frame feature: every destination receives one add per launch and launches are
stream-ordered, so the result does not depend on arrival order).  Scenes: 1500 Gaussians at 100 x 60 with an opaque disc (pixels
there stop early) and 64 Gaussians at 32 x 32; queries: points on eighths with points outside the image, a NaN and an inf, the
image corners, a 5 x 5 window of integer pixels on the dense spot and a 9 x 9 quarter-pixel grid inside one tile (more than 64 live
corners for one owner).  Digested: out, corner_T, corner_ncontrib of _forward and _forward_live for C = 1, 3, 65, 150, 300 (1, 1, 2,
3 accumulators per lane and two launches) and of _forward_batch (F = 3, a frame without queries, a query no frame owns); every
gradient of _backward_ordered, and of _backward_batch_ordered through FrameBatch.render_dynamic_sets(points=dict(..., ordered=True))
with a shared and a per-frame feature, with and without detach_opacity, for C = 1, 3, 70, 300; every gradient of _backward and
_backward_batch on the one-writer inputs.  On the opaque scene some walked list must exceed 64 entries (a second entry block)
and some corner must stop below its list length."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGEST_SB = 128          # QuarterCfg::SB, the longest super-batch among the quarter-list kernels
SCENES = {"dense": 20000, "sparse": 50}
W, H, F = 250, 187, 2


def _cases():
    out = []
    for C in (1, 3):
        for ab in (False, True):
            out.append(dict(name=f"narrow_c{C}_{'abs' if ab else 'noabs'}", kind="render", C=C, abs=ab))
    for C in (16, 19, 24, 32):
        out.append(dict(name=f"wide_c{C}", kind="render", C=C, abs=False))
    out.append(dict(name="sets_3_1_19_fwdrec", kind="sets", width=19, std=1))
    out.append(dict(name="sets_3_1_19_generic", kind="sets", width=19, std=0))
    out.append(dict(name="sets_3_1_4", kind="sets", width=4, std=1))
    out.append(dict(name="sets_3_1_8", kind="sets", width=8, std=1))
    out.append(dict(name="sets_3_1_19_l1_fused", kind="sets", width=19, std=1, l1=True))
    return out


def _points_queries(W, H, hx, hy):
    """the query points of the `points` family around the dense spot (hx, hy): float32 [Q, 2]"""
    import numpy as np
    nan, inf = float("nan"), float("inf")
    rng = np.random.default_rng(3)
    pts = [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [W - 1.5, H - 1.5], [W - 1, H - 1.25],       # the image corners
           [15.5, 15.5], [15, 16], [16, 15], [15.875, 15.125], [hx + 0.5, hy + 0.25], [hx - 0.875, hy + 0.5],
           [-0.5, 3], [W - 0.5, 5.25], [3.5, -0.125], [-0.25, -0.25], [W - 0.125, -0.875],                 # partly outside
           [-1, 2], [W, 3], [2, H], [-5, -5], [1e9, 2], [3e38, 1], [nan, 3], [3, nan], [inf, 2], [2, -inf]]   # outside, not finite
    pts += (np.round(rng.uniform(0, [W - 1, H - 1], size=(24, 2)) * 8) / 8).tolist()                      # on eighths
    pts += [[x, y] for y in range(hy - 2, hy + 3) for x in range(hx - 2, hx + 3) if 0 <= x < W and 0 <= y < H]
    tx, ty = min(hx // 16, (W - 8) // 16), min(hy // 16, (H - 8) // 16)
    q = 0.25 * np.arange(9)
    pts += np.stack(np.meshgrid(tx * 16 + 4 + q, ty * 16 + 4 + q), -1).reshape(-1, 2).tolist()             # 225 live corners, one tile
    return np.asarray(pts, np.float32)


def _points_family(record):
    import numpy as np
    import torch
    import dptr.gs as gs
    from splatter_a_video_amd import _lib as L
    from splatter_a_video_amd import train_step as TS
    from splatter_a_video_amd.dynamics import GAUSSIAN_MAJOR, FrameClock, frame_table, positions_batch_forward
    from splatter_a_video_amd.frames import FrameBatch
    from splatter_a_video_amd.gs.raster_ops import _points_forward, _points_inputs
    from splatter_a_video_amd.synth import make_scene

    def t(a, dtype=np.float32):
        return torch.tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")

    def digest(x):
        return hashlib.sha256(x.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

    def dense_spot(uv, W, H):
        hist, xe, ye = np.histogram2d(uv[:, 0], uv[:, 1], bins=[W // 4, H // 4], range=[[0, W], [0, H]])
        bx, by = np.unravel_index(np.argmax(hist), hist.shape)
        return int(xe[bx] + 2), int(ye[by] + 2)

    def put(name, res):
        record["cases"]["points/" + name] = res
        print(f"points/{name}: {len(res)} digests", flush=True)

    # ---- single frame
    scenes = {"opaque_100x60": (make_scene(1500, 100, 60, seed=21, clustered=0.4, cluster_area=0.03, blobs=1), 100, 60),
              "64_32x32": (make_scene(64, 32, 32, seed=12), 32, 32)}
    for sname, (sc, Ws, Hs) in scenes.items():
        N = sc.N
        uv, depth, conic, radius, tiles = gs.preprocess_ortho(t(sc.xyz), t(sc.scale), t(sc.rotate), t(sc.extr), Ws, Hs, nearest=0.01)
        hx, hy = dense_spot(uv.cpu().numpy(), Ws, Hs)
        op = sc.opacity.copy()
        if sname == "opaque_100x60":
            u = uv.cpu().numpy()
            op[(u[:, 0] - hx) ** 2 + (u[:, 1] - hy) ** 2 < 64] = 0.99
        op = t(op)
        idx, tr = gs.sort_gaussian(uv, depth, Ws, Hs, radius, tiles)
        pts_np = _points_queries(Ws, Hs, hx, hy)
        pts, one = t(pts_np), t([[hx, hy]])
        for C in (1, 3, 65, 150, 300):
            feat = t(np.random.default_rng(C).uniform(-1, 1, size=(N, C)))
            tensors, sizes = _points_inputs(uv, conic, op, feat, idx, tr, Ws, Hs, pts)
            res = {}
            for tag, live in (("", False), ("live_", True)):
                out, cT, cn = _points_forward(tensors, sizes, 0.75, True, live)
                res.update({tag + "out": digest(out), tag + "corner_T": digest(cT), tag + "corner_ncontrib": digest(cn)})
                if not live and C == 3 and sname == "opaque_100x60":   # what the walks cover, from the forward's own report
                    with np.errstate(invalid="ignore"):
                        x0, y0 = np.floor(pts_np[:, 0]), np.floor(pts_np[:, 1])
                        cx, cy = np.stack([x0, x0 + 1, x0, x0 + 1], 1), np.stack([y0, y0, y0 + 1, y0 + 1], 1)
                        inside = (cx >= 0) & (cx <= Ws - 1) & (cy >= 0) & (cy <= Hs - 1)
                    trn = tr.cpu().numpy().reshape(-1, 2)
                    tile = np.where(inside, cy, 0).astype(np.int64) // 16 * ((Ws + 15) // 16) + np.where(inside, cx, 0).astype(np.int64) // 16
                    n, last = (trn[:, 1] - trn[:, 0])[tile], cn.cpu().numpy()
                    res["longest_walked_list"], res["deepest_last"] = int(n[inside].max()), int(last[inside].max())
                    res["corners_stopped_early"] = int((inside & (last < n)).sum())
                    assert res["deepest_last"] > 64, f"no corner applies an entry past the first 64-entry block ({res['deepest_last']})"
                    assert res["corners_stopped_early"] >= 1, "no corner stops below its list length"
            put(f"{sname}/forward_c{C}", res)
        for C in (1, 3, 70, 300):
            rng = np.random.default_rng(100 + C)
            feat = t(rng.uniform(-1, 1, size=(N, C)))
            for tag, q, ordered in (("backward_ordered", pts, True), ("backward_atomic_one_writer", one, False)):
                g = t(np.random.default_rng(200 + C).normal(size=(q.shape[0], C)))
                lv = [x.detach().clone().requires_grad_(True) for x in (uv, conic, op, feat)]
                out = gs.alpha_blending_points(*lv, idx, tr, 0.75, Ws, Hs, q, differentiable=True, ordered=ordered)
                out.backward(g)
                torch.cuda.synchronize()
                res = {"out": digest(out)}
                res.update({"grad_" + k: digest(v.grad) for k, v in zip(("uv", "conic", "opacity", "feature"), lv)})
                assert all(float(v.grad.abs().max()) > 0 for v in lv), f"{sname}/{tag}_c{C}: a gradient is all zero"
                put(f"{sname}/{tag}_c{C}", res)

    # ---- the frame batch: F = 3, a frame without queries, a query no frame owns
    Nb, Wb, Hb, Tb, Fb = 1500, 100, 60, 20, 3
    sc = make_scene(Nb, Wb, Hb, F=Tb, seed=21, clustered=0.4, cluster_area=0.03, blobs=1)
    clock = FrameClock(Tb)
    p = TS.synthetic_video_params(sc, clock, "cuda", attrs=1, seed=22, cubic_sigma=0.01)
    uv = gs.preprocess_ortho(t(sc.xyz), t(sc.scale), t(sc.rotate), t(sc.extr), Wb, Hb, nearest=0.01)[0].cpu().numpy()
    hx, hy = dense_spot(uv, Wb, Hb)
    op = np.clip(sc.opacity.copy(), 1e-4, 1 - 1e-4)
    op[(uv[:, 0] - hx) ** 2 + (uv[:, 1] - hy) ** 2 < 64] = 0.99
    p["opacity"] = t(np.log(op / (1 - op))).reshape(p["opacity"].shape)
    rgb = t(np.random.default_rng(5).uniform(size=(Nb, 3)))
    extr = t(sc.extr)
    geom = ("pos_cubic_node", "rotation", "opacity", "scaling")

    def render(fb, leaves, points=None):
        sets = [dict(feature=rgb, bg=0.2, taps=True), dict(feature="depth", bg=1.0)]
        return fb.render_dynamic_sets(clock, [0, 7, 13], extr, sets, position=p["position"], pos_cubic_node=leaves["pos_cubic_node"],
                                      rotation=leaves["rotation"], rot_poly_feat=p["rot_poly_feat"],
                                      rot_fourier_feat=p["rot_fourier_feat"], opacity=leaves["opacity"], scaling=leaves["scaling"],
                                      cubic_layout=GAUSSIAN_MAJOR, K=8, points=points)

    def leaves():
        out = {k: p[k].detach().clone().requires_grad_(True) for k in geom}
        out["pos_cubic_node"] = p["pos_cubic_node"].detach().reshape(Nb, -1).clone().requires_grad_(True)
        return out

    f0 = _points_queries(Wb, Hb, hx, hy)
    f2 = np.asarray([[hx, hy], [40, 30], [20.375, 41.625], [Wb + 2.5, Hb + 1], [3, float("nan")]], np.float32)
    pts = t(np.concatenate([f0, f2, [[hx + 0.25, hy + 0.25]]]))             # the last query: nobody's
    off = torch.tensor([0, len(f0), len(f0), len(f0) + len(f2)], dtype=torch.int64, device="cuda")
    Q = pts.shape[0]
    one = t([[hx, hy]] * Fb)
    off_one = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device="cuda")
    g_img = [t(np.random.default_rng(9).normal(size=(Fb, c, Hb, Wb))) for c in (3, 1)]
    fb = FrameBatch(Fb, Nb, Wb, Hb, 4, "cuda")
    with torch.no_grad():
        render(fb, {k: v.detach() for k, v in leaves().items()})
    opa = torch.sigmoid(p["opacity"]).reshape(Nb, 1).contiguous()
    for C in (1, 3, 65, 150, 300):
        for per_frame in (False, True):
            feat = t(np.random.default_rng(300 + C).uniform(-1, 1, size=(Fb, Nb, C) if per_frame else (Nb, C)))
            out = torch.full((Q, C), 7.0, device="cuda")
            cT = torch.full((Q, 4), 7.0, device="cuda")
            cn = torch.full((Q, 4), 7, dtype=torch.int32, device="cuda")
            L.check(L.lib().splat_alpha_blending_points_forward_batch(
                Fb, Nb, C, L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(opa), 0, L.ptr(feat), Nb * C if per_frame else 0,
                L.ptr(fb.idx_sorted), L.ptr(fb.tile_range), fb.capacity, 0.75, Wb, Hb, Q, L.ptr(off),
                L.ptr(pts), L.ptr(out), L.ptr(cT), L.ptr(cn), L.stream()))
            torch.cuda.synchronize()
            assert float(out[-1].abs().max()) == 0 and int(cn[-1].abs().max()) == 0 and int(cn.max()) > 64
            put(f"batch/forward_c{C}_{'per_frame' if per_frame else 'shared'}",
                dict(out=digest(out), corner_T=digest(cT), corner_ncontrib=digest(cn)))
    for C in (1, 3, 70, 300):
        rng = np.random.default_rng(400 + C)
        shared, framed = t(rng.uniform(-1, 1, size=(Nb, C))), t(rng.uniform(-1, 1, size=(Fb, Nb, C)))
        # (the atomic route only where every destination has one writer per launch: one query per frame, a per-frame feature)
        runs = [(f"backward_ordered_c{C}_{'per_frame' if pf else 'shared'}_{'detach' if det else 'opacity'}", framed if pf else shared,
                 pts, off, True, det) for pf in (False, True) for det in (False, True)]
        runs += [(f"backward_atomic_one_writer_c{C}_{'detach' if det else 'opacity'}", framed, one, off_one, False, det)
                 for det in (False, True)]
        for name, feature, q, o, ordered, det in runs:
            lv = leaves()
            feat = feature.clone().requires_grad_(True)
            g = t(np.random.default_rng(500 + C).normal(size=(q.shape[0], C)))
            outs = render(fb, lv, points=dict(feature=feat, points=q, offsets=o, bg=0.0, detach_opacity=det, ordered=ordered))
            torch.autograd.backward(list(outs[:3]), [g_img[0], g_img[1], g])
            torch.cuda.synchronize()
            res = {"out": digest(outs[2]), "grad_feature": digest(feat.grad), "tap": digest(fb.tap)}
            res.update({"grad_" + k: digest(lv[k].grad) for k in geom})
            assert float(feat.grad.abs().max()) > 0
            put("batch/" + name, res)


def _child(out_path, family):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from splatter_a_video_amd import _lib as L
    from splatter_a_video_amd.frames import FrameBatch
    from splatter_a_video_amd.synth import make_scene

    def t(a, grad=False):
        return torch.tensor(np.asarray(a), device="cuda", requires_grad=grad)

    def digest(x):
        x = x.detach().contiguous().cpu().numpy()
        return hashlib.sha256(x.tobytes()).hexdigest()

    def batch_state(B, res):
        res["final_T"] = digest(B.final_T)
        res["ncontrib"] = digest(B.ncontrib)
        tr = B.tile_range.cpu().numpy()
        nc = B.ncontrib.cpu().numpy()
        res["tile_range"] = digest(B.tile_range)
        gx = (W + 15) // 16
        longest = 0
        for f in range(B.F):
            # The forward publishes a tile's words only as far as some pixel of the tile still applied an entry (the largest
            # ncontrib of the tile); the backward reads no further.  The rest of the buffer was never written: it is masked.
            words = B.cull_flags[f].cpu().numpy()
            written = np.zeros(words.size, bool)
            for t in range(tr.shape[1]):
                ys, xs = 16 * (t // gx), 16 * (t % gx)
                written[tr[f, t, 0]:tr[f, t, 0] + int(nc[f, ys:ys + 16, xs:xs + 16].max())] = True
            longest = max(longest, int((tr[f, :, 1] - tr[f, :, 0]).max()))
            res[f"cull_words_f{f}"] = hashlib.sha256(np.where(written, words, 0).tobytes()).hexdigest()
        res["tap"] = digest(B.tap)
        if B.abs_tap is not None:
            res["abs_tap"] = digest(B.abs_tap)
        return longest

    record = dict(build_id=L.build_id(), lib=os.path.basename(os.path.dirname(L.LIB_PATH)) + "/" + os.path.basename(L.LIB_PATH), cases={})
    for sname, N in SCENES.items() if family in ("all", "frames") else ():
        sc = make_scene(N, W, H, seed=7)
        off = t(np.stack([sc.positions(f) - sc.xyz for f in range(F)]).astype(np.float32))
        for case in _cases():
            rng = np.random.default_rng(11)
            res = {}
            geo = dict(xyz=sc.xyz, scales=sc.scale, uquats=sc.rotate, opacity=sc.opacity)
            if case["kind"] == "render":
                C = case["C"]
                p = {k: t(v, True) for k, v in dict(geo, feature=rng.uniform(size=(N, C)).astype(np.float32)).items()}
                g = t(rng.normal(size=(F, C, H, W)).astype(np.float32))
                B = FrameBatch(F, N, W, H, C, "cuda", want_abs=case["abs"])
                out = B.render(p["xyz"], p["scales"], p["uquats"], p["opacity"], p["feature"], off, t(sc.extr), bg=0.1)
                out.backward(g)
                torch.cuda.synchronize()
                res["image"] = digest(out)
            else:
                wd = case["width"]
                L.set_option("sets_std", case["std"])
                p = {k: t(v, True) for k, v in dict(geo, rgb=rng.uniform(size=(N, 3)).astype(np.float32),
                                                    attrs=rng.uniform(-1, 1, size=(N, wd)).astype(np.float32)).items()}
                imgs = [t(rng.normal(size=(F, c, H, W)).astype(np.float32)) for c in (3, 1, wd)]
                B = FrameBatch(F, N, W, H, 4 + wd, "cuda", want_abs=True)
                sets = [dict(feature=p["rgb"], bg=0.2, taps=True), dict(feature="depth", bg=1.0),
                        dict(feature=p["attrs"], bg=0.0, detach_opacity=True)]
                o = B.render_sets(p["xyz"], p["scales"], p["uquats"], p["opacity"], sets, off, t(sc.extr), K=20)
                if case.get("l1"):   # imgs are the targets; the kernel derives the gradient images
                    sums = torch.empty(F, B.T, 3, dtype=torch.float32, device="cuda")
                    B.fuse_l1(imgs, [0.8, 0.3, 0.5], sums)
                    torch.autograd.backward(list(o[:3]), B.l1_placeholders([3, 1, wd]))
                    torch.cuda.synchronize()
                    res["l1_tile_sums"] = digest(sums)
                else:
                    torch.autograd.backward(list(o[:3]), imgs)
                    torch.cuda.synchronize()
                L.set_option("sets_std", 1)
                for k, v in zip(("image_rgb", "image_depth", "image_attrs", "gs_idx"), o):
                    res[k] = digest(v)
            B.check()
            for k, v in p.items():
                res["grad_" + k] = digest(v.grad)
            longest = batch_state(B, res)
            res["longest_tile_list"] = longest
            if sname == "dense":
                assert longest > 2 * LARGEST_SB, f"{case['name']}: longest tile list {longest} <= two super-batches of {LARGEST_SB}"
            record["cases"][f"{sname}/{case['name']}"] = res
            print(f"{sname}/{case['name']}: longest tile list {longest}", flush=True)
    if family in ("all", "points"):
        _points_family(record)
    with open(out_path, "w") as fh:
        json.dump(record, fh, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", help="library of build A (e.g. the parent commit's)")
    ap.add_argument("--b", help="library of build B")
    ap.add_argument("--out", default="compare_builds.json")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child")
    ap.add_argument("--family", choices=("all", "frames", "points"), default="all",
                    help="frames: the frame-batch compositing cases; points: the sparse compositing at query points")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        _child(a.child, a.family)
        return 0
    if not a.a or not a.b:
        ap.error("--a and --b are required")
    sides = {}
    for tag, lib in (("a", a.a), ("b", a.b)):
        tmp = f"{a.out}.{tag}.tmp"
        env = dict(os.environ, SPLAT_LIB_PATH=os.path.abspath(lib))
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--family", a.family, "--child", tmp], env=env, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            rc = f"no status within {a.timeout} s (killed)"
        if rc != 0:   # a fault, abort, assertion or hang in a child ends the comparison: nothing more is started
            print(f"build {tag} ({lib}): child exited with {rc}", file=sys.stderr)
            return 2
        with open(tmp) as fh:
            sides[tag] = json.load(fh)
        os.remove(tmp)
    diff = []
    for case, ra in sides["a"]["cases"].items():
        rb = sides["b"]["cases"][case]
        diff += [f"{case}:{k}" for k in ra if ra[k] != rb.get(k)]
    ndig = sum(len(v) for v in sides["a"]["cases"].values())
    rec = dict(family=a.family)
    if a.family in ("all", "frames"):
        rec["scene"] = dict(W=W, H=H, F=F, gaussians=SCENES)
    if a.family in ("all", "points"):
        rec["points_scenes"] = {"opaque_100x60": dict(W=100, H=60, gaussians=1500), "64_32x32": dict(W=32, H=32, gaussians=64),
                                "batch": dict(W=100, H=60, F=3, gaussians=1500)}
    stamp_path = os.path.join(ROOT, "tools", ".stamp.json")   # the commit the tree was at (tools/stamp.py write), if recorded
    if os.path.exists(stamp_path):
        with open(stamp_path) as fh:
            st = json.load(fh)
        rec.update(git_head=st.get("git_head"), git_dirty=st.get("git_dirty"))
    rec.update(build_a=sides["a"]["build_id"], build_b=sides["b"]["build_id"], cases=len(sides["a"]["cases"]), digests_per_build=ndig,
               differing=diff, equal=not diff, digests=sides["a"]["cases"])
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(dict(build_a=rec["build_a"], build_b=rec["build_b"], cases=rec["cases"], digests=ndig, differing=diff)))
    return 0 if not diff else 1


if __name__ == "__main__":
    sys.exit(main())
