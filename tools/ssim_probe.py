"""SSIM / D-SSIM at the training step's size (25 frames x 3 x 480 x 854, both plane layouts): the fused HIP path (losses.ssim
forward + backward, losses.dssim_l1 forward + backward) against the same objective in eager float32 conv2d on the same GPU, and
TrainingStep(timing=True).phases()["loss"] at LossWeights.dssim = 0 and 0.2 on bench.py's training scene (GPU box).
HIP events around `--repeat` iterations after `--warmup`; prints one JSON line (and writes it with --out)."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as Fn

from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import losses
from splatter_a_video_amd import train_step as TS
from splatter_a_video_amd.dynamics import FrameClock
from splatter_a_video_amd.synth import make_scene


def eager_ssim(img1, img2, ws=11):
    """the reference's _ssim (src/pointrix/model/loss.py:58-112) in eager float32: five grouped conv2d"""
    C = img1.shape[-3]
    g = torch.tensor([math.exp(-(x - ws // 2) ** 2 / (2 * 1.5 ** 2)) for x in range(ws)], dtype=torch.float32)
    g = g / g.sum()
    w = (g[:, None] @ g[None, :]).to(img1.device).expand(C, 1, ws, ws).contiguous()
    conv = lambda t: Fn.conv2d(t, w, padding=ws // 2, groups=C)
    mu1, mu2 = conv(img1), conv(img2)
    s1, s2, s12 = conv(img1 * img1) - mu1 ** 2, conv(img2 * img2) - mu2 ** 2, conv(img1 * img2) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))).mean()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--step-repeat", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_probe needs a GPU")
    dev = torch.device("cuda:0")
    F, H, W = a.frames, 480, 854
    gen = torch.Generator(device=dev).manual_seed(0)
    gt = torch.rand(F, 3, H, W, device=dev, generator=gen)
    pred0 = (gt + 0.1 * torch.randn(F, 3, H, W, device=dev, generator=gen)).clamp(0, 1)
    rec = {"build_id": L.build_id(), "shape": [F, 3, H, W], "warmup": a.warmup, "repeat": a.repeat}
    for layout in ("reference", "image"):
        view = lambda t: losses.planes(t, layout)
        pred = pred0.clone().requires_grad_(True)

        def fused_ssim():
            s = losses.ssim(view(pred), view(gt))
            torch.autograd.grad(s, [pred])

        def fused_dssim():
            d = losses.dssim_l1(pred, gt, 0.2, layout)
            torch.autograd.grad(d, [pred])

        def eager_ssim_fb():
            s = eager_ssim(view(pred), view(gt))
            torch.autograd.grad(s, [pred])

        def eager_dssim():
            d = 0.8 * (pred - gt).abs().mean() + 0.2 * (1 - eager_ssim(view(pred), view(gt)))
            torch.autograd.grad(d, [pred])

        r = {k: round(timed(f, a.warmup, a.repeat), 4) for k, f in
             (("ssim_fwd_bwd_ms", fused_ssim), ("dssim_l1_fwd_bwd_ms", fused_dssim), ("eager_ssim_fwd_bwd_ms", eager_ssim_fb),
              ("eager_dssim_l1_fwd_bwd_ms", eager_dssim))}
        r["speedup_ssim"] = round(r["eager_ssim_fwd_bwd_ms"] / r["ssim_fwd_bwd_ms"], 2)
        r["speedup_dssim_l1"] = round(r["eager_dssim_l1_fwd_bwd_ms"] / r["dssim_l1_fwd_bwd_ms"], 2)
        with torch.no_grad():
            r["ssim_fused"] = float(losses.ssim(view(pred), view(gt)))
            r["ssim_eager_f32"] = float(eager_ssim(view(pred), view(gt)))
        rec[layout] = r
    del pred0, gt
    torch.cuda.empty_cache()
    # the training step's loss phase at lambda 0 / 0.2: bench.py --train-step's scene and frames
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
    lr = {k: 1e-6 for k in TS.REFERENCE_LR}
    steps = {}
    for lam in (0.0, 0.2):
        st = TS.TrainingStep(start, clock, W, H, F, extr, lr=lr, K=20, weights=TS.LossWeights(dssim=lam), timing=True)
        st.step(t1, t2, gts)
        acc, tot = [], []
        for _ in range(a.step_repeat):
            st.step(t1, t2, gts)
            ph = st.phases()
            acc.append(ph["loss"])
            tot.append(sum(ph.values()))
        steps[str(lam)] = {"loss_phase_ms": round(sorted(acc)[len(acc) // 2], 4), "step_ms": round(sorted(tot)[len(tot) // 2], 3),
                           "loss": st.loss()}
        del st
        torch.cuda.empty_cache()
    steps["loss_phase_added_ms"] = round(steps["0.2"]["loss_phase_ms"] - steps["0.0"]["loss_phase_ms"], 4)
    rec["train_step"] = steps
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
