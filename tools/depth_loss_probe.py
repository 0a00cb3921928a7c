"""The median-normalised depth loss at the training step's size (25 frames of 854 x 480): the HIP path
(splat_depth_dpt_loss_grad: loss only, loss + gradient image, the same with cached ground-truth statistics, losses.depth_loss_dpt
forward + backward) against the float32 eager restatement of tests/depth_ref.py on the same GPU, forward + backward, and
TrainingStep(timing=True) on bench.py's training scene with the default weights and with LossWeights.depth_dpt = 1.0 (GPU box).
HIP events around `--repeat` iterations after `--warmup`; prints one JSON line (and writes it with --out).

`--root TREE --default-step-only`: the default step of ANOTHER checkout of the project (its package and its built library), to
compare against the parent commit in the same session."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--step-repeat", type=int, default=7)
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--default-step-only", action="store_true")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


ARGS = _args()
sys.path.insert(0, os.path.abspath(ARGS.root))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import train_step as TS
from splatter_a_video_amd.dynamics import FrameClock
from splatter_a_video_amd.synth import make_scene


def timed(fn, warmup, repeat):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeat):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeat


def depth_images(F, H, W, dev):
    """a rendered depth with the blend's background plateau (bg = 1.0 on 30 % of the pixels, so the median lies below it) and
    an unrelated monocular prior of another scale and shift"""
    gen = torch.Generator(device=dev).manual_seed(0)
    y = torch.linspace(0, 1, H, device=dev)[:, None]
    x = torch.linspace(0, 1, W, device=dev)[None, :]
    pred = (0.2 + 0.5 * x + 0.2 * torch.sin(5 * y) + 0.05 * torch.randn(F, 1, H, W, device=dev, generator=gen)).clamp(0.05, 0.95)
    pred[torch.rand(F, 1, H, W, device=dev, generator=gen) < 0.3] = 1.0
    gt = 2.0 - 1.5 * y + 0.3 * torch.cos(4 * x) + 0.2 * torch.randn(F, 1, H, W, device=dev, generator=gen)
    return pred.contiguous(), gt.contiguous()


def kernel_times(a, dev):
    from depth_ref import restate
    from splatter_a_video_amd import losses
    F, H, W = a.frames, 480, 854
    pred, gt = depth_images(F, H, W, dev)
    per = torch.empty(F, device=dev)
    g = torch.empty(F, 1, H, W, device=dev)
    gs = losses.depth_stats(gt)
    p = pred.clone().requires_grad_(True)

    def autograd_fn():
        torch.autograd.grad(losses.depth_loss_dpt(p, gt), [p])

    def eager():
        img = pred.detach().clone().requires_grad_(True)
        ls = [restate(img[f], gt[f]) for f in range(F)]
        torch.autograd.grad(torch.stack(ls).mean(), [img])
        return ls

    r = {"loss_only_ms": timed(lambda: losses.depth_dpt_loss_grad(pred, gt, per_frame=per), a.warmup, a.repeat),
         "loss_and_grad_ms": timed(lambda: losses.depth_dpt_loss_grad(pred, gt, 1.0, g, per_frame=per), a.warmup, a.repeat),
         "loss_only_cached_gt_ms": timed(lambda: losses.depth_dpt_loss_grad(pred, gt, per_frame=per, gt_stats=gs), a.warmup,
                                         a.repeat),
         "loss_and_grad_cached_gt_ms": timed(lambda: losses.depth_dpt_loss_grad(pred, gt, 1.0, g, per_frame=per, gt_stats=gs),
                                             a.warmup, a.repeat),
         "depth_stats_ms": timed(lambda: losses.depth_stats(gt), a.warmup, a.repeat),
         "depth_loss_dpt_fwd_bwd_ms": timed(autograd_fn, a.warmup, a.repeat),
         "eager_fwd_bwd_ms": timed(eager, 2, 5)}
    r = {k: round(v, 4) for k, v in r.items()}
    r["speedup_vs_eager"] = round(r["eager_fwd_bwd_ms"] / r["depth_loss_dpt_fwd_bwd_ms"], 1)
    ties = torch.empty(F, dtype=torch.int32, device=dev)
    losses.depth_dpt_loss_grad(pred, gt, per_frame=per, ties=ties)
    want = torch.stack([x.detach() for x in eager()])
    r["max_rel_loss_diff_vs_eager"] = float(((per - want).abs() / want.abs()).max())
    r["ties_min_max"] = [int(ties.min()), int(ties.max())]
    return r


def step_times(a, dev, configs):
    F, H, W = a.frames, 480, 854
    sc = make_scene(a.gaussians, W, H, F=50, C=0, seed=1234)
    clock = FrameClock(sc.F)
    truth = TS.synthetic_video_params(sc, clock, dev, attrs=16)
    extr = torch.tensor(sc.extr, device=dev)
    t1 = list(range(F))
    t2 = [int((17 * t + 11) % sc.F) for t in t1]
    t2 = [t if t != u else (t + 1) % sc.F for t, u in zip(t2, t1)]
    gts = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
    g2 = torch.Generator(device=dev).manual_seed(7)
    start = {k: v.clone() for k, v in truth.items()}
    for k, sg in (("shs", 0.1), ("attrs", 0.2), ("opacity", 0.3), ("scaling", 0.05)):
        start[k] = start[k] + sg * torch.randn(start[k].shape, device=dev, generator=g2)
    start["pos_cubic_node"] = torch.zeros_like(start["pos_cubic_node"])
    del truth
    # the depth prior: another frame's depth, mirrored, at another scale and shift (not the rendered depth itself)
    gts["depth"] = (3.0 * gts["depth"].roll(1, 0).flip(-1) - 0.5).contiguous()
    lr = {k: 1e-6 for k in TS.REFERENCE_LR}
    steps = {}
    for name, kw in configs:
        st = TS.TrainingStep(start, clock, W, H, F, extr, lr=lr, K=20, weights=TS.LossWeights(**kw), timing=True)
        st.step(t1, t2, gts)
        st.step(t1, t2, gts)
        acc, tot = [], []
        for _ in range(a.step_repeat):
            st.step(t1, t2, gts)
            ph = st.phases()
            acc.append(ph["loss"])
            tot.append(sum(ph.values()))
        steps[name] = {"loss_phase_ms": round(sorted(acc)[len(acc) // 2], 4), "step_ms": round(sorted(tot)[len(tot) // 2], 3),
                       "step_ms_min_max": [round(min(tot), 3), round(max(tot), 3)], "loss": st.loss()}
        if "depth_dpt" in st.last:
            steps[name]["depth_dpt"] = float(st.last["depth_dpt"])
        del st
        torch.cuda.empty_cache()
    return steps


def main():
    a = ARGS
    if not torch.cuda.is_available():
        raise SystemExit("depth_loss_probe needs a GPU")
    dev = torch.device("cuda:0")
    rec = {"build_id": L.build_id(), "frames": a.frames, "size": [480, 854], "warmup": a.warmup, "repeat": a.repeat,
           "step_repeat": a.step_repeat}
    if a.default_step_only:
        rec["train_step"] = step_times(a, dev, [("default", {})])
    else:
        rec["kernel"] = kernel_times(a, dev)
        torch.cuda.empty_cache()
        steps = step_times(a, dev, [("default", {}), ("depth_dpt1", dict(depth_dpt=1.0)),
                                    ("depth_dpt1_only", dict(depth=0.0, depth_dpt=1.0)), ("default_again", {})])
        steps["step_added_ms"] = round(steps["depth_dpt1"]["step_ms"] - steps["default"]["step_ms"], 3)
        rec["train_step"] = steps
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
