"""Golden vectors for the median-normalised depth loss from the reference's own ``depth_loss_dpt`` (src/loss.py:184-207), called
on the CPU as the trainer calls it (src/trainer_fragGS.py:600: two [H, W, 1] tensors, no weight).  Values AND autograd gradients
w.r.t. the rendered depth.  Data only travels.

    python tests/golden/make_golden_depth.py    ->  tests/golden/depth_loss.npz

Cases (40 x 56 except ``odd``): ``smooth`` (ramps + noise); ``plateau`` (more than half of the rendered pixels exactly 1.0, the
depth blend's background: the median sits inside the plateau); ``odd`` (39 x 55: the other parity of n); ``signed`` (gt a
disparity with both signs and a few exact zeros of both signs, a pred with both signs too); ``nan`` (one NaN in the rendered
depth: loss and every gradient element are NaN).
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import torch

REF = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("smooth", "plateau", "odd", "signed", "nan")


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _ramp(rng, H, W, lo, hi):
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    a, b, c = rng.uniform(-1, 1, 3)
    z = a * x + b * y + c * np.sin(3 * x + 2 * y) + rng.normal(0, 0.4, (H, W))
    return (lo + (hi - lo) * (z - z.min()) / (z.max() - z.min())).astype(np.float32)


def _case(kind, rng):
    H, W = (39, 55) if kind == "odd" else (40, 56)
    pred, gt = _ramp(rng, H, W, 0.5, 5.0), _ramp(rng, H, W, 0.2, 3.0)
    if kind == "plateau":
        pred = _ramp(rng, H, W, 0.1, 0.95)
        pred[rng.random((H, W)) < 0.6] = 1.0
    if kind == "signed":
        pred = rng.normal(0, 1, (H, W)).astype(np.float32)
        gt = rng.normal(0.2, 2, (H, W)).astype(np.float32)
        idx = rng.choice(H * W, 12, replace=False)
        gt.reshape(-1)[idx[:6]] = 0.0
        gt.reshape(-1)[idx[6:]] = -0.0
    if kind == "nan":
        pred[H // 3, W // 2] = np.nan
    return pred, gt


def main():
    ref = _load("ref_loss", "loss.py")
    rng = np.random.default_rng(2025)
    out = {}
    for kind in CASES:
        pred, gt = _case(kind, rng)
        p = torch.from_numpy(pred)[..., None].clone().requires_grad_(True)          # [H, W, 1], as the trainer passes it
        loss = ref.depth_loss_dpt(p, torch.from_numpy(gt)[..., None])
        (g,) = torch.autograd.grad(loss, [p])
        out[f"{kind}_pred"], out[f"{kind}_gt"] = pred, gt
        out[f"{kind}_loss"] = np.float32(loss.detach())
        out[f"{kind}_grad"] = g[..., 0].numpy().astype(np.float32)
        print(kind, float(loss.detach()), int((torch.from_numpy(pred) == torch.median(torch.from_numpy(pred))).sum()))
    np.savez_compressed(os.path.join(HERE, "depth_loss.npz"), **out)


if __name__ == "__main__":
    main()
