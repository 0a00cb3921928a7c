"""Seeding the dynamic Gaussians from a clip's 2-D tracks, depth and masks on the GPU.

What the reference runs on the CPU before its first training step, as native kernels (csrc/seed.hip):

* ``median_filter_2d`` / ``depth_from_disparity``   the 11x11 median of every depth map
  (reference: src/video3Dflow/utils.py:198-210, src/video3Dflow/video_3d_flow.py:131-137);
* ``normalize_depths`` / ``lift_tracks`` / ``extend_tracks_3d``   TAPIR tracks lifted to 3-D through the depth maps and
  filtered by the masks (video_3d_flow.py:48-94,164-248, utils.py:53-174);
* ``fit_cubic_nodes``   one not-a-knot cubic spline per Gaussian and coordinate
  (src/dynamic_gaussian_with_base_point_cloud.py:55-78, a scipy call per point there);
* ``seed_dynamic_gaussians``   the parameter set ``DynamicGaussians`` / ``TrainingStep`` run on, scales from the 3-nearest-
  neighbour distance (src/pointrix/utils/gaussian_points/gaussian_utils.py:68-100).

Reading files, eroding the masks and the random choice of tracks stay with the caller: every function takes tensors.
There is no CPU fallback, and no kernel here uses float atomics (all of it runs under ``set_deterministic(True)``).
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .dynamics import FrameClock
from .knn import distCUDA2

LiftedTracks = namedtuple("LiftedTracks", "tracks_3d colors visibles invisibles confidences")

MAX_KNOTS = 64      # SPLAT_SPLINE_MAX_KNOTS (include/splat_hip.h): 63 segments, a clip of ~315 frames with the default clock
SH_C0 = 0.28209479177387814


def median_filter_2d(x: Tensor, kernel_size: int = 11) -> Tensor:
    """``median_filter_2d(x, kernel_size, 1)`` of the reference (same=True): reflect padding of ``kernel_size // 2`` and the
    element of rank ``(k*k-1)/2`` of every k x k window -- a selection, bit-equal to the reference.  ``x`` is [B,C,H,W] or
    [T,H,W] float32; k odd in 3..11; H and W greater than ``k // 2``.  NaN is not an input the filter orders."""
    if not isinstance(x, Tensor) or x.dim() not in (3, 4):
        raise ValueError("x must be [B, C, H, W] or [T, H, W]")
    k = int(kernel_size)
    if k != kernel_size or k < 3 or k > 11 or k % 2 == 0:
        raise ValueError("kernel_size must be odd, 3..11")
    H, W = int(x.shape[-2]), int(x.shape[-1])
    xc = L.need(x, "x")
    P = xc.numel() // max(H * W, 1)
    if P > 0 and (H <= k // 2 or W <= k // 2):
        raise ValueError("H and W must exceed kernel_size // 2 (reflect padding)")
    out = torch.empty_like(xc)
    L.check(L.lib().splat_median_filter_2d(P, H, W, k, L.ptr(xc), L.ptr(out), L.stream()))
    return out


def depth_from_disparity(disp: Tensor) -> Tensor:
    """a depth map as the reference loads it (video_3d_flow.py:131-137): ``1 / clip(disp, 1e-6, 1e6)``, then the 11x11
    median.  ``disp`` [H,W], [T,H,W] or [B,C,H,W]."""
    if not isinstance(disp, Tensor) or disp.dim() not in (2, 3, 4):
        raise ValueError("disp must be [H, W], [T, H, W] or [B, C, H, W]")
    d = L.need(disp, "disp")
    depth = 1.0 / torch.clamp(d, 1e-6, 1e6)
    return median_filter_2d(depth[None] if depth.dim() == 2 else depth, 11).reshape(d.shape)


def normalize_depths(depths: Tensor, lo: float = 0.5, hi: float = 2.0) -> Tuple[Tensor, Tensor, Tensor]:
    """the clip's depths scaled to [lo, hi] (video_3d_flow.py:61-64); returns (depths', min, max), min and max as 0-dim
    device tensors (``extend_tracks_3d`` takes them)."""
    d = L.need(depths, "depths")
    dmin, dmax = d.min(), d.max()
    return (d - dmin) / (dmax - dmin) * (hi - lo) + lo, dmin, dmax


def _lift(tracks_2d: Tensor, depths: Tensor, masks: Tensor, query_index: int, query_img: Tensor, grid_coords: bool):
    tr = L.need(tracks_2d, "tracks_2d")
    dp = L.need(depths, "depths")
    mk = L.need(masks, "fg_masks")
    im = L.need(query_img, "query_img")
    if tr.dim() != 3 or tr.shape[2] != 4:
        raise ValueError("tracks_2d must be [N, T, 4]")
    N, T = int(tr.shape[0]), int(tr.shape[1])
    if dp.dim() != 3 or dp.shape[0] != T:
        raise ValueError("depths must be [T, H, W] with the tracks' T")
    H, W = int(dp.shape[1]), int(dp.shape[2])
    if tuple(mk.shape) != (T, H, W):
        raise ValueError("fg_masks must be [T, H, W] like depths")
    if tuple(im.shape) != (H, W, 3):
        raise ValueError("query_img must be [H, W, 3]")
    if T > 0 and not 0 <= int(query_index) < T:
        raise ValueError("query_index outside the clip")
    dev = tr.device
    t3 = torch.empty(N, T, 3, dtype=torch.float32, device=dev)
    col = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    vis = torch.zeros(N, T, dtype=torch.uint8, device=dev)
    inv = torch.zeros(N, T, dtype=torch.uint8, device=dev)
    conf = torch.zeros(N, T, dtype=torch.float32, device=dev)
    inm = torch.zeros(N, T, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(N, 2, dtype=torch.int32, device=dev)
    L.check(L.lib().splat_lift_tracks(N, T, H, W, L.ptr(tr), L.ptr(dp), L.ptr(mk), query_index,
                                      L.ptr(im), 1 if grid_coords else 0, L.ptr(t3), L.ptr(col), L.ptr(vis), L.ptr(inv),
                                      L.ptr(conf), L.ptr(inm), L.ptr(cnt), L.stream()))
    return t3, col, vis.bool(), inv.bool(), conf, inm.bool(), cnt


def _count_rule(counts: Tensor, thr: float, T: int) -> Tensor:
    # counts >= min(int(thr * T), quantile(counts, thr))   (utils.py:137-158); N integers, on the host like the reference's
    c = counts.cpu()
    return (c >= min(int(thr * T), c.float().quantile(thr).item())).to(counts.device)


def lift_tracks(tracks_2d: Tensor, depths: Tensor, fg_masks: Tensor, query_index: int, query_img: Tensor,
                extract_fg: bool = True, return_valid: bool = False):
    """``get_tracks_3d_for_query_frame(query_index, query_img, tracks_2d, depths, fg_masks, extract_fg)`` of the reference:
    ``tracks_2d`` [N,T,4] (x, y, occlusion logit, expected-distance logit), ``depths`` / ``fg_masks`` [T,H,W], ``query_img``
    [H,W,3].  One kernel does the per-(track, frame) work and the per-track counts; the ``valid`` rule (in the mask at the
    query frame, visible and confident often enough) is torch on the counts and synchronises with the host once.  Returns
    ``LiftedTracks`` of the n valid tracks (and the [N] bool ``valid`` with ``return_valid``)."""
    t3, col, vis, inv, conf, inm, cnt = _lift(tracks_2d, depths, fg_masks, query_index, query_img, False)
    N, T = int(t3.shape[0]), int(t3.shape[1])
    if N == 0 or T == 0:
        valid = torch.zeros(N, dtype=torch.bool, device=t3.device)
    else:
        thr = 0.9 if extract_fg else 0.99
        valid = inm[:, int(query_index)] & _count_rule(cnt[:, 0], thr, T) & _count_rule(cnt[:, 1], thr, T)
    out = LiftedTracks(t3[valid], col[valid], vis[valid], inv[valid], conf[valid])
    return (out, valid) if return_valid else out


def extend_tracks_3d(tracks_3d: Tensor, depth0: Tensor, depthL: Tensor, img0: Tensor, imgL: Tensor, mask0: Tensor,
                     maskL: Tensor, depth_min: Tensor, depth_max: Tensor, grid_size: int = 64, margin: float = 0.25,
                     lo: float = 0.5, hi: float = 2.0) -> Tuple[Tensor, Tensor]:
    """``Video3DFlow.extend_track3d`` (video_3d_flow.py:164-248): a grid of points on the left border of the first frame and
    on the right border of the last one, kept where the mask sample is NOT 1, lifted through the un-normalised depth
    (``depth0`` / ``depthL`` [H,W], then scaled with ``depth_min`` / ``depth_max`` of ``normalize_depths``) and moved by the mean
    displacement of ``tracks_3d`` [N,T,3] relative to that frame.  Returns (points [M,T,3], colors [M,3])."""
    tr = L.need(tracks_3d, "tracks_3d")
    if tr.dim() != 3 or tr.shape[2] != 3:
        raise ValueError("tracks_3d must be [N, T, 3]")
    d0 = L.need(depth0, "depth0")
    if d0.dim() != 2:
        raise ValueError("depth0 must be [H, W]")
    H, W = int(d0.shape[0]), int(d0.shape[1])
    dev = tr.device
    wh = torch.tensor([W, H])[None]
    ny = H // int(grid_size * margin)
    spans = [(0, int((W - 1) * margin)), (int((W - 1) * (1 - margin)), W - 1)]
    dmin, dmax = torch.as_tensor(depth_min, device=dev), torch.as_tensor(depth_max, device=dev)
    pts, cols = [], []
    for (x_lo, x_hi), depth, img, mask, ref in zip(spans, (d0, depthL), (img0, imgL), (mask0, maskL), (0, -1)):
        # the grid is a handful of points: built on the host with the reference's own calls (float32 linspace), then uploaded
        grid = torch.meshgrid(torch.linspace(x_lo, x_hi, W // grid_size), torch.linspace(0, H - 1, ny), indexing="ij")
        p2 = (torch.stack(grid, dim=-1).reshape(-1, 2) - wh / 2) / (wh / 2)
        M = p2.shape[0]
        q = torch.zeros(M, 1, 4, dtype=torch.float32)
        q[:, 0, :2] = p2
        t3, col, _, _, _, inm, _ = _lift(q.to(dev), L.need(depth, "depth")[None], L.need(mask, "mask")[None], 0, img, True)
        keep = ~inm[:, 0]
        p3 = t3[keep, 0].clone()
        p3[:, 2] = (p3[:, 2] - dmin) / (dmax - dmin) * (hi - lo) + lo
        delta = (tr - tr[:, ref:][:, :1]).mean(dim=0, keepdim=True, dtype=torch.float64).float()
        pts.append(p3[:, None] + delta)
        cols.append(col[keep])
    return torch.cat(pts, dim=0), torch.cat(cols, dim=0)


def knot_frames(clock: FrameClock, T: int) -> np.ndarray:
    """frame index of every knot of ``clock`` in a clip of T frames: ``round(intervals * (T - 1))``"""
    return np.rint(clock.intervals.astype(np.float64) * (T - 1)).astype(np.int32)


def fit_cubic_nodes(tracks_3d: Tensor, clock: Optional[FrameClock] = None) -> Tuple[Tensor, Tensor, FrameClock]:
    """``position`` [N,3] (the frame-0 point) and ``pos_cubic_node`` [N, 4*I*3] (the reference's [N,4,I,3], highest power
    first: ``scipy.interpolate.CubicSpline(clock.intervals, y).c`` with y = the track minus its frame-0 point at the knot
    frames) of ``tracks_3d`` [N,T,3]; ``clock`` defaults to ``FrameClock(T)``.  Not-a-knot at both ends; 2 knots give a line,
    3 knots the parabola through them.  A float64 solve rounded once to float32, like the reference's.  At most
    ``MAX_KNOTS`` knots, strictly increasing, each on a frame of the clip."""
    tr = L.need(tracks_3d, "tracks_3d")
    if tr.dim() != 3 or tr.shape[2] != 3 or tr.shape[1] < 1:
        raise ValueError("tracks_3d must be [N, T, 3]")
    N, T = int(tr.shape[0]), int(tr.shape[1])
    if clock is None:
        clock = FrameClock(T)
    if clock.num_frames != T:
        raise ValueError(f"the clock counts {clock.num_frames} frames, the tracks have {T}")
    knots =np.ascontiguousarray(clock.intervals, dtype=np.float32)
    n = int(knots.size)
    if n < 2 or n > MAX_KNOTS:
        raise ValueError(f"a spline needs 2..{MAX_KNOTS} knots, got {n}")
    if not np.all(np.diff(knots.astype(np.float64)) > 0):
        raise ValueError("knots must be strictly increasing")
    frames = np.ascontiguousarray(knot_frames(clock, T))
    if frames.min() < 0 or frames.max() >= T:
        raise ValueError("a knot lies on a frame outside the clip")
    I = n - 1
    position = torch.empty(N, 3, dtype=torch.float32, device=tr.device)
    cubic = torch.empty(N, 4 * I * 3, dtype=torch.float32, device=tr.device)
    L.check(L.lib().splat_fit_cubic_nodes(N, T, n, knots.ctypes.data_as(ctypes.c_void_p),
                                          frames.ctypes.data_as(ctypes.c_void_p), L.ptr(tr), L.ptr(position), L.ptr(cubic),
                                          L.stream()))
    return position, cubic, clock


def seed_dynamic_gaussians(tracks_3d: Tensor, clock: Optional[FrameClock] = None, colors: Optional[Tensor] = None,
                           init_opacity: float = 0.5, attrs: int = 16,
                           generator: Optional[torch.Generator] = None) -> Tuple[Dict[str, Tensor], FrameClock]:
    """the parameter set of the reference's point cloud at its set-up (dynamic_gaussian_with_base_point_cloud.py:55-78 with
    gaussian_utils.py:68-100), keys and shapes of ``train_step.synthetic_video_params``: tracks with a NaN in any frame are
    dropped; ``position`` / ``pos_cubic_node`` from ``fit_cubic_nodes``; ``scaling`` = log sqrt of the clamped mean squared
    3-nearest-neighbour distance, three times; unit ``rotation``; ``opacity`` = logit(init_opacity); zero rotation tables,
    ``attrs`` and higher SH bands; SH DC = ``(colors - 0.5) / C0`` when ``colors`` [N,3] is given, else ``rand / 255`` from
    ``generator`` (the reference's ``get_random_feauture``)."""
    tr = L.need(tracks_3d, "tracks_3d")
    if tr.dim() != 3 or tr.shape[2] != 3 or tr.shape[1] < 1:
        raise ValueError("tracks_3d must be [N, T, 3]")
    if not 0.0 < float(init_opacity) < 1.0:
        raise ValueError("init_opacity must lie in (0, 1)")
    if colors is not None:
        colors = L.need(colors, "colors")
        if tuple(colors.shape) != (tr.shape[0], 3):
            raise ValueError("colors must be [N, 3]")
    keep = ~torch.isnan(tr).any(dim=2).any(dim=1)
    tr = tr[keep].contiguous()
    dev = tr.device
    position, cubic, clock = fit_cubic_nodes(tr, clock)
    N = int(position.shape[0])
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    if N > 0:
        scaling = torch.log(torch.sqrt(torch.clamp_min(distCUDA2(position), 1e-7)))[:, None].repeat(1, 3)
    else:
        scaling = z(0, 3)
    rotation = z(N, 4)
    rotation[:, 0] = 1.0
    shs = z(N, 16, 3)
    if colors is not None:
        shs[:, 0, :] = (colors[keep] - 0.5) / SH_C0
    else:
        gdev = generator.device if generator is not None else dev
        shs[:, 0, :] = torch.rand(N, 3, dtype=torch.float32, device=gdev, generator=generator).to(dev) / 255.0
    params = {"position": position, "pos_cubic_node": cubic, "rotation": rotation, "rot_poly_feat": z(N, 4, 4),
              "rot_fourier_feat": z(N, 8, 4), "opacity": torch.full((N, 1), math.log(init_opacity / (1.0 - init_opacity)),
                                                                    dtype=torch.float32, device=dev),
              "scaling": scaling.contiguous(), "shs": shs, "attrs": z(N, int(attrs))}
    return params, clock
