"""Point tracking on the native path: where does pixel ``p`` of frame ``i`` go in every other frame?

The reference answers with one full render of frame ``i`` per target frame ``t`` -- the per-Gaussian feature ``pixel_flow =
uv_t - uv_i`` (``draw_pixel_trajectory``, src/trainer_fragGS.py:1483-1566, called from src/train.py:98 and the trainer's ``log``,
:911) or ``track_gs`` (``get_correspondences_and_occlusion_masks_for_pixels_core``, :1644-1677) -- and an ``F.grid_sample`` of each
image at the query points.  The compositing weights of frame ``i`` do not depend on ``t``; only the feature does.  ``track_pixels``
therefore walks the tile lists of frame ``i`` once, at the four bilinear corner pixels of every query only, and composites ONE wide
feature row per query that holds all target frames side by side:

    frame_preprocess + sort_gaussian of the query frame, splat_track_flow_rows, splat_alpha_blending_points_forward

-- four native steps whatever the number of target frames.  Orthographic camera only (the reference's tracker projects with the
renderer's ortho ``project_point``).  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .dynamics import GAUSSIAN_MAJOR, SEGMENT_MAJOR, DynamicGaussians, FrameClock, frame_preprocess, frame_table
from .gs.raster_ops import alpha_blending_points, sort_gaussian

_NAMES = ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")


class Tracks(NamedTuple):
    """``tracks`` [T, Q, 2] pixel positions of the queries at every target time; ``track_depth`` [T, Q] the composited depth of
    the tracked surface there (background 0); ``alpha`` [Q] = 1 - the sampled final transmittance of the query frame;
    with ``occlusion=True`` also ``surface_depth`` [T, Q], the target frame's own depth render (background 1) at the tracked
    points, and ``occluded`` [T, Q] = ``surface_depth >= track_depth`` (else both None)."""
    tracks: Tensor
    track_depth: Tensor
    alpha: Tensor
    surface_depth: Optional[Tensor] = None
    occluded: Optional[Tensor] = None


# (W, H, device) -> the two float32 factors of sample_coords on that device.  Lives as long as the module; 8 bytes per entry, and
# cleared when more than 16 frame sizes have been seen, so it cannot grow with a caller that sweeps sizes.
_SCALES: Dict[tuple, Tensor] = {}


def sample_coords(points_px: Tensor, W: int, H: int) -> Tensor:
    """Where a pixel coordinate is sampled -- THE DEFINITION used by ``track_pixels``:

        ix = px * float32((W - 1) / W),    iy = py * float32((H - 1) / H)        (one float32 multiply each)

    The reference normalises with ``normalize_coords`` (src/util.py:65-72: ``2 p / (W, H) - 1``) and samples with
    ``align_corners=True``, which maps [-1, 1] onto [0, W - 1]: ``ix = ((2 px / W - 1) + 1) / 2 * (W - 1)``; the formula above is
    that map in one rounding.  ``ix`` is grid_sample's un-normalised column index (``gs.alpha_blending_points``)."""
    key = (int(W), int(H), str(points_px.device))
    s = _SCALES.get(key)
    if s is None:      # created once per (W, H, device): a host-to-device copy per call otherwise
        if len(_SCALES) >= 16:
            _SCALES.clear()
        s = torch.tensor([np.float32((W - 1) / W), np.float32((H - 1) / H)], dtype=torch.float32, device=points_px.device)
        _SCALES[key] = s
    return points_px * s


def _cull_args(nearest: float, extent: float):
    """nearest = extent = 0 switches culling off.  splat_track_flow_rows has a real switch for it; the per-frame preprocess has
    none and gets limits no finite point reaches instead.  The two are not exactly equivalent: a point whose depth is NaN (read as
    0) or clamped to -FLT_MAX (an infinite z) is still culled by the preprocess (depth <= -3e38 fails only for finite depths), and
    so is one more than 1e30 frame widths off screen, while the rows kernel keeps all of them.  Such a Gaussian is absent from the
    rendered frame either way (it reaches no tile), so the difference never enters a composited value."""
    if nearest == 0 and extent == 0:
        return -3.0e38, 1.0e30
    return float(nearest), float(extent)


@torch.no_grad()
def track_pixels(model: Union[Dict[str, Tensor], DynamicGaussians], clock: FrameClock, ref_time, points_px: Tensor,
                 times: Sequence[float], extr: Tensor, W: int, H: int, nearest: float = 0.01, extent: float = 1.3,
                 occlusion: bool = False, cubic_layout: Optional[int] = None) -> Tracks:
    """Track ``points_px`` [Q, 2] (pixel coordinates (x, y) of frame ``ref_time``) to every time of ``times``.

    ``model``: a ``DynamicGaussians`` or a dict with position [N,3], pos_cubic_node, rotation [N,4], rot_poly_feat [N,4,4],
    rot_fourier_feat [N,8,4], opacity [N,1] (logit), scaling [N,3] (log) -- the parameters ``TrainingStep`` trains
    (``cubic_layout``: layout of a dict's pos_cubic_node, default the reference's [N, 4*I*3]; ``TrainingStep`` stores it
    segment-major).  ``extr``: the orthographic camera [3|4, 4].

    * ``tracks[t]`` = ``points_px`` + the composited flow ``uv_t - uv_ref`` of frame ``ref_time`` sampled at the queries: ``px2s``
      of src/trainer_fragGS.py:1541.  Sampling positions: ``sample_coords``.
    * ``track_depth[t]``: the composited depth (orthographic z at time t, background 0) of what the query pixel shows.
    * ``alpha``: 1 - the sampled final transmittance (sampled with zero padding like everything else: a query outside the frame
      reads transmittance 0).
    * a Gaussian culled at time t (``nearest`` / ``extent`` as in the renderer's ``project_point``) enters with uv_t = depth_t = 0,
      as in the reference; ``nearest = extent = 0`` switches culling off, for the query frame too.
    * ``occlusion=True`` adds per target frame that frame's preprocess, sort and one sparse compositing of its depth
      (background 1, the renderer's depth blend) at the tracked points: ``surface_depth`` and ``occluded = surface_depth >=
      track_depth`` (:1665-1676).  The tracked points are mapped by ``sample_coords`` like the queries (the reference hands
      un-normalised pixels to that one grid_sample: INTEGRATION.md).

    Memory: the feature rows are written for ALL N Gaussians and all T target times, 12 N T bytes (180 MB at 300k Gaussians and
    50 frames), although the walk reads only the Gaussians listed in the queried tiles; for a long clip call with ``times`` in
    chunks (every call repeats the query frame's preprocess and sort, which is cheap next to gigabytes of rows).
    """
    if isinstance(model, DynamicGaussians):
        p = {k: getattr(model, k).detach() for k in _NAMES}
        layout = model.cubic_layout if cubic_layout is None else int(cubic_layout)
    else:
        p = {k: model[k].detach() for k in _NAMES}
        layout = GAUSSIAN_MAJOR if cubic_layout is None else int(cubic_layout)
    if layout not in (GAUSSIAN_MAJOR, SEGMENT_MAJOR):
        raise ValueError("cubic_layout must be GAUSSIAN_MAJOR or SEGMENT_MAJOR")
    W, H = int(W), int(H)
    points_px = L.need(points_px, "points_px")
    if points_px.dim() != 2 or points_px.shape[1] != 2:
        raise ValueError("points_px must have shape [Q, 2] = (x, y)")
    times = list(times)
    T, Q = len(times), points_px.shape[0]
    if T < 1:
        raise ValueError("times must name at least one target frame")
    position = L.need(p["position"], "position")
    N, I = position.shape[0], clock.interval_num
    cubic = L.need(p["pos_cubic_node"], "pos_cubic_node")
    if cubic.numel() != N * 4 * I * 3:
        raise ValueError("pos_cubic_node must hold N * 4 * interval_num * 3 floats")
    extr_c = L.need(extr, "extr")
    dev = position.device
    near_p, ext_p = _cull_args(nearest, extent)

    def preprocess(time):
        uv, depth, conic, radius, tiles, opa = frame_preprocess(
            clock, time, extr_c, W, H, position=position, pos_cubic_node=cubic, rotation=p["rotation"],
            rot_poly_feat=p["rot_poly_feat"], rot_fourier_feat=p["rot_fourier_feat"], opacity=p["opacity"], scaling=p["scaling"],
            nearest=near_p, extent=ext_p, cubic_layout=layout)
        idx_sorted, tile_range = sort_gaussian(uv, depth, W, H, radius, tiles)
        return uv, depth, conic, opa, idx_sorted, tile_range

    uv, _, conic, opa, idx_sorted, tile_range = preprocess(ref_time)
    rows = torch.empty(N, T, 3, dtype=torch.float32, device=dev)
    tab = frame_table(clock, times, dev)
    L.check(L.lib().splat_track_flow_rows(
        T, N, I, L.ptr(tab), L.ptr(position), L.ptr(cubic), layout, L.ptr(extr_c), W, H,
        nearest, extent, L.ptr(uv), L.ptr(rows), L.stream()))
    pts = sample_coords(points_px, W, H)
    out = alpha_blending_points(uv, conic, opa, rows.view(N, 3 * T), idx_sorted, tile_range, 0.0, W, H, pts)
    out = out.view(Q, T, 3).permute(1, 0, 2)
    tracks = points_px[None] + out[..., :2]
    track_depth = out[..., 2].contiguous()
    # the sampled final transmittance from the same kernel: a zero feature over background 1 composites to sum_k w_k T_k
    alpha = 1.0 - alpha_blending_points(uv, conic, opa, torch.zeros(N, 1, dtype=torch.float32, device=dev), idx_sorted, tile_range,
                                        1.0, W, H, pts)[:, 0]
    if not occlusion:
        return Tracks(tracks, track_depth, alpha)
    surface = torch.empty(T, Q, dtype=torch.float32, device=dev)
    for t, time in enumerate(times):
        uv_t, depth_t, conic_t, opa_t, idx_t, tr_t = preprocess(time)
        surface[t] = alpha_blending_points(uv_t, conic_t, opa_t, depth_t.view(N, 1), idx_t, tr_t, 1.0, W, H,
                                           sample_coords(tracks[t].contiguous(), W, H))[:, 0]
    return Tracks(tracks, track_depth, alpha, surface, surface >= track_depth)
