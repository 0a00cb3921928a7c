"""The track term's blend, dense against sparse, at the c2 scene (300k Gaussians, 854 x 480, SURVEY 8d generator): a 3-channel
feature composited and back-propagated for Q unique integer query pixels, Q = 1024, 4096, 16384.

  dense    gs.alpha_blending forward + backward with a gradient image that is zero off the query pixels (the route the training
           step takes today: the whole image is composited and replayed, the loss reads Q pixels of it)
  sparse   gs.alpha_blending_points(differentiable=True) forward + backward (splat_alpha_blending_points_forward / _backward):
           only the query pixels walk their tile lists
  ordered  the same with ordered=True (splat_alpha_blending_points_backward_ordered): no float atomic, the tile owns its corners

--crowded K adds one case per K: K sub-pixel queries inside a 48 x 48 pixel window (nine tiles), where one wave of the ordered
backward walks hundreds of corners one after the other (no dense leg's gradient image there: the dense leg is skipped).

Both return the gradients w.r.t. uv, conic and the feature; the opacity is detached, as the reference does for this blend.  The
two routes are timed in alternating rounds in one process with device events around a window of consecutive forward + backward
calls and a synchronise behind it (ms per call; median, minimum and maximum over the rounds), after warming both up at every Q.
Their gradients are compared at every Q with the project's gradient criterion.  One JSON record (with the commit stamp of
tools/stamp.py and the build id) goes to --out.

    python tools/track_sparse_bench.py [--rounds 10] [--out profiles/points_backward_bench.json]
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
from splatter_a_video_amd.synth import make_scene  # noqa: E402
from stamp import stamp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--calls", type=int, default=20, help="forward + backward calls inside one timed window")
ap.add_argument("--gaussians", type=int, default=300000)
ap.add_argument("--queries", type=int, nargs="+", default=[1024, 4096, 16384])
ap.add_argument("--crowded", type=int, nargs="*", default=[4096])
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "points_backward_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("track_sparse_bench needs the GPU: a timing taken anywhere else says nothing")

N, W, H, C = args.gaussians, 854, 480, 3
dev = torch.device("cuda:0")
t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
sc = make_scene(N, W, H, seed=1234)
uv0, depth, conic0, radius, tiles = gs.preprocess_ortho(t(sc.xyz), t(sc.scale), t(sc.rotate), t(sc.extr), W, H, nearest=0.01)
idx, tr = gs.sort_gaussian(uv0, depth, W, H, radius, tiles)
opacity = t(sc.opacity)
rng = np.random.default_rng(7)
feat0 = t(rng.uniform(-1, 1, size=(N, C)))
uv, conic, feat = (x.detach().clone().requires_grad_(True) for x in (uv0, conic0, feat0))
leaves = (uv, conic, feat)


def case(Q, crowded=False):
    g = torch.tensor(rng.normal(size=(Q, C)).astype(np.float32), device=dev)
    if crowded:
        points = torch.tensor((np.array([400.0, 224.0]) + rng.uniform(0, 48, size=(Q, 2))).astype(np.float32), device=dev)
        gimg = None
    else:
        pix = torch.tensor(np.sort(rng.choice(W * H, size=Q, replace=False)), device=dev)
        points = torch.stack([pix % W, pix // W], 1).to(torch.float32)
        gimg = torch.zeros(C, H * W, device=dev).index_copy(1, pix, g.t().contiguous()).view(C, H, W)

    def dense():
        img = gs.alpha_blending(uv, conic, opacity, feat, idx, tr, 0.0, W, H)
        return torch.autograd.grad(img, leaves, gimg)

    def sparse():
        out = gs.alpha_blending_points(uv, conic, opacity, feat, idx, tr, 0.0, W, H, points, differentiable=True)
        return torch.autograd.grad(out, leaves, g)

    def ordered():
        out = gs.alpha_blending_points(uv, conic, opacity, feat, idx, tr, 0.0, W, H, points, differentiable=True, ordered=True)
        return torch.autograd.grad(out, leaves, g)

    return (None if crowded else dense), sparse, ordered


def timed(fn, calls):
    """ms per call of `calls` consecutive calls inside one window"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def grad_ratio(got, ref):
    """largest |got - ref| / (2 (2e-3 |ref| + 1e-4 max |ref|)) over the elements of the three gradients"""
    worst = 0.0
    for a, b in zip(got, ref):
        a, b = a.double(), b.double()
        lim = 2 * (2e-3 * b.abs() + 1e-4 * b.abs().max())
        worst = max(worst, float(((a - b).abs() / lim).max()))
    return worst


stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "rounds": len(v)}
cases = []
def kernels(fn, names, reps=5):
    """per-kernel events: a pass of its own (the brackets cost host time)"""
    L.profile_enable(True)
    L.profile_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    kern = {}
    for name in names:       # (prefix match: "blend_points" holds every kernel of the route)
        total, launches = L.profile_read(name)
        kern[name] = {"ms_per_call": total / reps, "launches_per_call": launches / reps}
    L.profile_enable(False)
    return kern


for Q, crowded in [(q, False) for q in args.queries] + [(q, True) for q in args.crowded]:
    dense, sparse, ordered = case(Q, crowded)
    for _ in range(3):      # warm up every shape of the timed window
        a, b, c = (dense() if dense else None), sparse(), ordered()
    torch.cuda.synchronize()
    ms = {"dense": [], "sparse": [], "ordered": []}
    for _ in range(args.rounds):
        if dense:
            ms["dense"].append(timed(dense, args.calls))
        ms["sparse"].append(timed(sparse, args.calls))
        ms["ordered"].append(timed(ordered, args.calls))
    bits = all(torch.equal(x, y) for x, y in zip(c, ordered()))
    rec = {"queries": Q, "crowded_into_48x48_pixels": crowded, "sparse_points_fwd_bwd": stat(ms["sparse"]),
           "ordered_points_fwd_bwd": stat(ms["ordered"]),
           "ordered_over_sparse_median": float(np.median(ms["ordered"]) / np.median(ms["sparse"])),
           "sparse_kernels": kernels(sparse, ("blend_points_bwd", "blend_points")),
           "ordered_kernels": kernels(ordered, ("blend_points_bwd_ord", "blend_points_ord_lists", "blend_points_ord_zero",
                                                "blend_points_ord_gauss", "blend_points")),
           "ordered_bit_equal_run_to_run": bits, "ordered_gradient_error_over_bound_vs_sparse": grad_ratio(c, b)}
    if dense:
        rec.update({"dense_alpha_blending_fwd_bwd": stat(ms["dense"]),
                    "dense_over_sparse_median": float(np.median(ms["dense"]) / np.median(ms["sparse"])),
                    "gradient_error_over_bound": grad_ratio(b, a)})
    print(json.dumps(rec), flush=True)
    cases.append(rec)

rec = {"bench": "points_backward", **stamp(), "device": torch.cuda.get_device_name(0), "gaussians": N, "W": W, "H": H, "channels": C,
       "cases": cases, "calls_per_window": args.calls,
       "timing": "device events around a window of consecutive forward + backward calls + synchronise, ms per call; windows of the "
                 "routes alternate in one process after 3 warm-up calls of each at every Q; kernel times from the library's own "
                 "per-kernel events in a pass of their own, not a tracer",
       "gradient_error_over_bound": "largest |sparse - dense| / (2 (2e-3 |dense| + 1e-4 max |dense|)) over uv, conic and feature"}
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
