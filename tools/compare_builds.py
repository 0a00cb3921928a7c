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
the empty-tile exit and the zero-record path)."""
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


def _child(out_path):
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
    for sname, N in SCENES.items():
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
    with open(out_path, "w") as fh:
        json.dump(record, fh, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", help="library of build A (e.g. the parent commit's)")
    ap.add_argument("--b", help="library of build B")
    ap.add_argument("--out", default="compare_builds.json")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        _child(a.child)
        return 0
    if not a.a or not a.b:
        ap.error("--a and --b are required")
    sides = {}
    for tag, lib in (("a", a.a), ("b", a.b)):
        tmp = f"{a.out}.{tag}.tmp"
        env = dict(os.environ, SPLAT_LIB_PATH=os.path.abspath(lib))
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], env=env, timeout=a.timeout).returncode
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
    rec = dict(scene=dict(W=W, H=H, F=F, gaussians=SCENES), build_a=sides["a"]["build_id"], build_b=sides["b"]["build_id"],
               cases=len(sides["a"]["cases"]), digests_per_build=ndig, differing=diff, equal=not diff, digests=sides["a"]["cases"])
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(dict(build_a=rec["build_a"], build_b=rec["build_b"], cases=rec["cases"], digests=ndig, differing=diff)))
    return 0 if not diff else 1


if __name__ == "__main__":
    sys.exit(main())
