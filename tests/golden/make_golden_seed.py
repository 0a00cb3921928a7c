"""Golden vectors for the seeding stage (splatter_a_video_amd/seed.py) from the reference's own functions:
``median_filter_2d`` and ``get_tracks_3d_for_query_frame`` (src/video3Dflow/utils.py:69-174,198-210) imported from its
tree, ``Video3DFlow.extend_track3d`` (src/video3Dflow/video_3d_flow.py:164-248) called unbound on a namespace that carries
what the method reads, and ``scipy.interpolate.CubicSpline`` as src/dynamic_gaussian_with_base_point_cloud.py:66-78 calls
it.  Build container only (the reference tree is not present on the GPU box); the .npz it writes is what travels.

    python tests/golden/make_golden_seed.py <reference>/src

Contents of seed_clip.npz (numeric arrays only): a clip of T = 12 frames of 45 x 70 -- disparity (smooth + noise, frame 3
constant, frame 7 quantised to 8 levels: the median's tie cases), its median-filtered depth, the normalised depths, masks in
{-1, 0, 1}, three images, two query frames with 300 sub-pixel tracks each (some on integer pixels, some outside the image,
some across mask edges), lifted with both ``extract_fg`` values, the border extension, and the spline of one lifted set.

The generator resamples any track sample that breaks one of
  1. |visibility * confidence - 0.5| > 1e-5  and  |(1 - visibility) * confidence - 0.5| > 1e-5,
  2. |confidence - 0.5| > 1e-5,
  3. the pinned float32 bilinear formula (evaluated in numpy below) gives torch's in-mask decision,
so that no decision of the fixture hangs on the last bit of an exponential.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
T, H, W, N = 12, 45, 70, 300
QUERIES = (0, 7)


def _load_reference(ref_src):
    sys.path.insert(0, ref_src)
    for name in ("cv2", "imageio"):
        sys.modules.setdefault(name, types.ModuleType(name))
    import video3Dflow.utils as U
    spec = importlib.util.spec_from_file_location("ref_v3f", os.path.join(ref_src, "video3Dflow", "video_3d_flow.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return U, m.Video3DFlow


def pinned_bilinear_zero(img, x, y):
    """the pinned float32 formula of the in-mask sample: img [T,H,W], x / y [T,N] pixel coordinates -> [T,N]"""
    f = np.float32
    Tn, Hh, Ww = img.shape
    gx = x.astype(f) / f(Ww - 1) * f(2) - f(1)
    gy = y.astype(f) / f(Hh - 1) * f(2) - f(1)
    ix = ((gx + f(1)) / f(2)) * f(Ww - 1)
    iy = ((gy + f(1)) / f(2)) * f(Hh - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + f(1), y0 + f(1)
    nw, ne, sw, se = (x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)
    tt = np.arange(Tn)[:, None]
    acc = np.zeros_like(ix, dtype=f)
    for w, xs, ys in ((nw, x0, y0), (ne, x1, y0), (sw, x0, y1), (se, x1, y1)):
        ok = (xs >= 0) & (xs <= Ww - 1) & (ys >= 0) & (ys <= Hh - 1)
        v = img[tt, np.clip(ys, 0, Hh - 1).astype(np.int64), np.clip(xs, 0, Ww - 1).astype(np.int64)]
        acc = np.where(ok, acc + w * v, acc).astype(f)
    return acc


def make_clip(rng):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    disp = np.empty((T, H, W), np.float32)
    for t in range(T):
        smooth = 0.6 + 0.3 * np.sin(xx / 9.0 + 0.3 * t) * np.cos(yy / 7.0 - 0.2 * t)
        disp[t] = smooth + 0.05 * rng.normal(size=(H, W))
    disp[3] = 0.8                                                     # constant frame: every window is one tie
    disp[7] = np.round(disp[7] * 8.0) / 8.0 + 0.125                   # 8 levels: ties at the median rank
    disp = np.clip(disp, 0.05, None).astype(np.float32)
    # a foreground disc that drifts to the right, a band of 0 around it (the eroded border), background -1
    cx = 22.0 + 2.0 * np.arange(T)
    cy = 22.0 + 0.5 * np.arange(T)
    masks = np.empty((T, H, W), np.float32)
    for t in range(T):
        r = np.hypot(xx - cx[t], yy - cy[t])
        masks[t] = np.where(r < 11.0, 1.0, np.where(r < 14.0, 0.0, -1.0))
    imgs = rng.uniform(size=(T, H, W, 3)).astype(np.float32)
    return disp, masks, imgs, cx, cy


def make_tracks(rng, q, cx, cy):
    """[N,T,4]: 45 % ride the disc, 35 % rest on the background, the rest wander; a tenth on integer pixels, some outside"""
    x0 = np.empty(N)
    y0 = np.empty(N)
    kind = rng.choice(3, size=N, p=[0.45, 0.35, 0.20])
    ang, rad = rng.uniform(0, 2 * np.pi, N), 12.5 * np.sqrt(rng.uniform(size=N))      # across the disc's rim too
    x0[:] = np.where(kind == 0, cx[q] + rad * np.cos(ang), rng.uniform(-3.0, W + 2.0, N))
    y0[:] = np.where(kind == 0, cy[q] + rad * np.cos(ang + 1.0), rng.uniform(-3.0, H + 2.0, N))
    tr = np.empty((N, T, 4), np.float32)
    for t in range(T):
        dx = np.where(kind == 0, cx[t] - cx[q], np.where(kind == 1, 0.0, 1.5 * (t - q)))
        dy = np.where(kind == 0, cy[t] - cy[q], np.where(kind == 1, 0.0, -0.7 * (t - q)))
        tr[:, t, 0] = x0 + dx + 0.05 * rng.normal(size=N)
        tr[:, t, 1] = y0 + dy + 0.05 * rng.normal(size=N)
    on_pixel = rng.uniform(size=N) < 0.1
    tr[on_pixel, :, :2] = np.round(tr[on_pixel, :, :2])
    tr[:, :, 2] = rng.normal(-4.0, 2.5, size=(N, T))                   # occlusion logit: mostly visible
    tr[:, :, 3] = rng.normal(-4.0, 2.5, size=(N, T))                   # expected-distance logit: mostly confident
    return tr


def settle(rng, U, tr, fg_masks_both):
    """resample the samples that break conditions 1-3 (module docstring) until none does"""
    for _ in range(100):
        t4 = torch.from_numpy(tr).swapaxes(0, 1)                       # [T,N,4]
        vis = 1 - torch.sigmoid(t4[..., 2])
        conf = 1 - torch.sigmoid(t4[..., 3])
        bad = ((vis * conf - 0.5).abs() <= 1e-5) | (((1 - vis) * conf - 0.5).abs() <= 1e-5) | ((conf - 0.5).abs() <= 1e-5)
        bad = bad.numpy().T                                            # [N,T]
        tr[bad, 2:] = rng.normal(-4.0, 2.5, size=(int(bad.sum()), 2)).astype(np.float32)
        bad_pos = np.zeros((N, T), bool)
        for m in fg_masks_both:
            ref = F.grid_sample(torch.from_numpy(m)[:, None], U.normalize_coords(t4[:, None, :, :2], H, W),
                                align_corners=True)[:, 0, 0] == 1
            mine = pinned_bilinear_zero(m, tr[:, :, 0].T, tr[:, :, 1].T) == 1
            bad_pos |= (ref.numpy() != mine).T
        tr[bad_pos, :2] += rng.uniform(-0.3, 0.3, size=(int(bad_pos.sum()), 2)).astype(np.float32)
        if not bad.any() and not bad_pos.any():
            return tr
    raise RuntimeError("could not settle the track samples")


def valid_rows(U, tr, t3):
    """which of the N tracks the reference kept (it returns them in order): match the normalised 2-D trajectories"""
    wh = torch.tensor([W, H])[None]
    allxy = ((torch.from_numpy(tr)[..., :2] - wh / 2) / (wh / 2)).numpy()
    valid = np.zeros(N, bool)
    j = 0
    for i in range(N):
        if j < t3.shape[0] and np.array_equal(allxy[i], t3[j, :, :2]):
            valid[i] = True
            j += 1
    assert j == t3.shape[0], "could not recover the reference's valid rows"
    return valid


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    from scipy.interpolate import CubicSpline
    torch.manual_seed(0)
    torch.set_num_threads(1)
    U, Video3DFlow = _load_reference(sys.argv[1])
    rng = np.random.default_rng(2025)
    disp, masks, imgs, cx, cy = make_clip(rng)
    out = {"disp": disp, "masks": masks.astype(np.int8)}
    # depth maps as load_depth makes them (video_3d_flow.py:131-137), then get_tracks_3d's normalisation (:61-64)
    depth = torch.from_numpy((1.0 / np.clip(disp, a_min=1e-6, a_max=1e6))).float()
    depth_med = torch.stack([U.median_filter_2d(depth[t][None, None], 11, 1)[0, 0] for t in range(T)])
    dmin, dmax = depth_med.min(), depth_med.max()
    depths = (depth_med - dmin) / (dmax - dmin) * (2.0 - 0.5) + 0.5
    out.update(depth_med=depth_med.numpy(), depths=depths.numpy(), depth_min=dmin.numpy(), depth_max=dmax.numpy())
    keep_imgs = sorted(set(QUERIES) | {0, T - 1})
    out["img_frames"] = np.array(keep_imgs, np.int32)
    out["imgs"] = imgs[keep_imgs]
    fg = {1: (masks == 1).astype(np.float32), 0: (masks == -1).astype(np.float32)}
    first = None
    for q in QUERIES:
        tr = settle(rng, U, make_tracks(rng, q, cx, cy), (fg[1], fg[0]))
        out[f"q{q}_tracks_2d"] = tr
        for efg in (1, 0):
            res = U.get_tracks_3d_for_query_frame(q, torch.from_numpy(imgs[q]), torch.from_numpy(tr), depths,
                                                  torch.from_numpy(fg[efg]), extract_fg=bool(efg))
            t3, col, vis, inv, conf = [r.numpy() for r in res]
            pre = f"q{q}_fg{efg}_"
            out.update({pre + "tracks_3d": t3, pre + "colors": col, pre + "visibles": vis, pre + "invisibles": inv,
                        pre + "confidences": conf, pre + "valid": valid_rows(U, tr, t3)})
            print(pre, "valid", t3.shape[0], "of", N)
            assert 10 <= t3.shape[0] < N
            if first is None:
                first = torch.from_numpy(t3)
    # the border extension on the first lifted set (grid_size 16: 4 x 11 grid points per side at 45 x 70)
    ns = types.SimpleNamespace(depths=[depth_med[t] for t in range(T)], depths_min=dmin, depths_max=dmax,
                               depth_range_min=0.5, depth_range_max=2.0,
                               get_depth=lambda i: depth_med[i], get_image=lambda i: torch.from_numpy(imgs[i]),
                               get_mask=lambda i: torch.from_numpy(masks[i]))
    ext_p, ext_c = Video3DFlow.extend_track3d(ns, first, grid_size=16, margin=0.25)
    out.update(ext_grid_size=np.int32(16), ext_margin=np.float32(0.25), ext_points=ext_p.numpy(), ext_colors=ext_c.numpy())
    print("extension", tuple(ext_p.shape))
    # the spline of that set, as the reference's setup fits it (:66-78)
    I = int(np.ceil(T / 5))
    idx = torch.linspace(0, T - 1, I + 1).long()
    xx = (idx / (T - 1)).numpy()
    delta = (first - first[:, :1]).numpy()
    coeff = np.array([CubicSpline(xx, yy).c for yy in delta[:, idx.numpy()]])       # [n, 4, I, 3]
    out.update(spline_intervals=xx.astype(np.float32), spline_coeff=coeff.astype(np.float32))
    path = os.path.join(HERE, "seed_clip.npz")
    np.savez_compressed(path, **out)
    print("seed_clip.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
