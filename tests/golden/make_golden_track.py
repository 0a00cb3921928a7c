"""Golden vectors for the 2-D track loss (the trainer's optical-flow term, src/trainer_fragGS.py:528-569) from the reference's
own ``parse_tapir_track_info`` (src/video3Dflow/utils.py:53-66), ``denormalize_coords`` (src/util.py:75-82) and
``masked_l1_loss`` (src/criterion.py:32-53), called on the CPU with the trainer's arguments (``mask`` and ``quantile=0.98``;
``normalize`` left at its default, True: the confidence-weighted mean of the kept residuals).  The modules' imports this container
lacks (``torchvision``, ``imageio``, ``cv2``) are stubbed; none of them is used by these functions.  Values AND autograd
gradients w.r.t. the rendered track image.  Data only travels.

    python tests/golden/make_golden_track.py    ->  tests/golden/track_loss.npz

Cases: ``grid`` (queries on a stride-4 grid in raster order), ``shuffled`` (the same kind of grid, fractional coordinates, the
file in random order: the raster-rank pairing), ``ties`` (invisible points, residuals on a 1/8 lattice with many exact ties,
some zero), ``nan`` (a NaN in the image at a visible query: the reference's loss and gradient are 0).
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _stubs():
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    for name in ("imageio", "cv2"):
        sys.modules[name] = types.ModuleType(name)


def flow_term(crit, util, vutils, img, query_xy, rows, t1, t2, num_imgs):
    """one pair of the trainer's flow term (src/trainer_fragGS.py:528-569), built from the reference's three functions with the
    trainer's arguments: img [1, C, h, w] (the rendered track_gs), query_xy [Q, 2], rows [1, Q, 4]; t1, t2 int64 [1]"""
    h, w = img.shape[-2:]
    pair_w = torch.exp(-2 * torch.abs(t2 - t1).float() / num_imgs)
    xy = util.denormalize_coords(img.permute(0, 2, 3, 1)[..., :2], h, w).reshape(h * w, 2)
    visible, _, conf = vutils.parse_tapir_track_info(rows[..., 2], rows[..., 3])
    visible, conf = visible.reshape(-1), conf.reshape(-1)
    # the prediction is gathered through a boolean mask over the raster: raster order, paired with the rows in file order
    at_query = torch.zeros(h * w, dtype=torch.bool)
    qi = query_xy.to(torch.int64)
    at_query[qi[:, 1] * w + qi[:, 0]] = True
    pred = xy[at_query][visible]
    if pred.shape[0] == 0:
        return img.sum() * 0.0
    # the trainer's call: no `normalize` argument, so masked_l1_loss's default (True) holds
    return crit.masked_l1_loss(pred, rows.reshape(-1, 4)[visible, :2], mask=(conf[:, None] * pair_w)[visible],
                               quantile=0.98) / max(h, w)


def _case(kind, rng):
    H, W = 40, 56
    f32 = np.float32
    ys, xs = np.meshgrid(np.arange(0, H, 4), np.arange(0, W, 4), indexing="ij")
    q = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(f32)
    Q = q.shape[0]
    if kind == "ties":
        track = (rng.integers(-64, 64, size=(1, 3, H, W)) / 64.0).astype(f32)         # X, Y on a lattice: exact
    else:
        track = rng.uniform(-1, 1, size=(1, 3, H, W)).astype(f32)
    X = ((track[0, 0] + f32(1)) * f32(W)) / f32(2)
    Y = ((track[0, 1] + f32(1)) * f32(H)) / f32(2)
    pi = q.astype(np.int64)
    tgt = np.zeros((Q, 4), f32)
    if kind == "ties":
        off = rng.integers(-3, 4, size=(Q, 2)) / 8.0
        off[rng.random(Q) < 0.2] = 0.0
        tgt[:, 0] = X[pi[:, 1], pi[:, 0]] + off[:, 0]
        tgt[:, 1] = Y[pi[:, 1], pi[:, 0]] + off[:, 1]
        tgt[:, 2] = np.where(rng.random(Q) < 0.3, 4.0, -5.0)        # a third occluded
        tgt[:, 3] = np.where(rng.random(Q) < 0.1, 3.0, -4.0)        # some unconfident
    else:
        noise = rng.normal(0, 2.0, size=(Q, 2))
        out = rng.random(Q) < 0.05
        noise[out] *= 15.0                                          # outliers above the 0.98 quantile
        tgt[:, 0] = X[pi[:, 1], pi[:, 0]] + noise[:, 0]
        tgt[:, 1] = Y[pi[:, 1], pi[:, 0]] + noise[:, 1]
        tgt[:, 2] = rng.normal(-2.0, 2.0, size=Q)
        tgt[:, 3] = rng.normal(-2.0, 2.0, size=Q)
    if kind == "nan":          # a diverged image: torch.quantile is NaN, nothing is kept, the loss is 0 / (0 + 1e-8) = 0
        v = int(np.nonzero((1 - 1 / (1 + np.exp(-tgt[:, 2]))) * (1 - 1 / (1 + np.exp(-tgt[:, 3]))) > 0.6)[0][0])
        track[0, 0, pi[v, 1], pi[v, 0]] = np.nan
    if kind == "shuffled":
        q = q + rng.uniform(0.0, 0.95, size=q.shape).astype(f32)      # truncated to the same pixels
        perm = rng.permutation(Q)
        q, tgt = q[perm], tgt[perm]
    ids1, ids2 = {"grid": (3, 11), "shuffled": (17, 2), "ties": (5, 6), "nan": (0, 9)}[kind]
    return dict(track=track, query_xy=q, target=tgt, ids1=np.int64(ids1), ids2=np.int64(ids2), num_imgs=np.int64(24))


def main():
    _stubs()
    sys.path.insert(0, REF)
    crit = _load("ref_criterion", "criterion.py")
    util = _load("ref_util", "util.py")
    vutils = _load("ref_video3dflow_utils", os.path.join("video3Dflow", "utils.py"))
    rng = np.random.default_rng(2024)
    out = {}
    for kind in ("grid", "shuffled", "ties", "nan"):
        c = _case(kind, rng)
        track = torch.from_numpy(c["track"]).requires_grad_(True)
        loss = flow_term(crit, util, vutils, track, torch.from_numpy(c["query_xy"]), torch.from_numpy(c["target"])[None],
                         torch.tensor([int(c["ids1"])]), torch.tensor([int(c["ids2"])]), int(c["num_imgs"]))
        (g,) = torch.autograd.grad(loss, [track])
        for k, v in c.items():
            out[f"{kind}_{k}"] = v
        out[f"{kind}_loss"] = np.float32(loss.detach())
        out[f"{kind}_grad"] = g.numpy().astype(np.float32)
        print(kind, float(loss.detach()), int((g != 0).sum()))
    np.savez_compressed(os.path.join(HERE, "track_loss.npz"), **out)


if __name__ == "__main__":
    main()
