"""Dense optical flow of the learned video: flow maps between any two frame times, their colours, their error.

The reference's ``get_pred_flows_gs`` (src/trainer_fragGS.py:777-821) projects every Gaussian at the frame times ``ids1`` and
``ids2``, composites ``uv2 - uv1`` over the sorted lists of frame ``ids1`` with the opacity detached and background 0
(dptr_ortho_enhanced.py:361-376) and colours the result with ``util.flow_to_image`` (src/util.py:421-536); its earlier flow
term ``masked_l1_loss(pred_flow, px2s - px1s, weights)`` survives as a comment (:525-526).

Here (csrc/flow.hip, include/splat_hip_flow.h): ``flow_attribute`` is the per-Gaussian ``uv2 - uv1`` of a batch of pairs in
one launch each way, ``render_flow`` composites it as a per-frame tensor of the detached set of
``FrameBatch.render_dynamic_sets`` (the clip mechanics of ``views.render_views``), ``flow_to_image`` is the Middlebury
colouring on the device, ``flow_epe`` / ``losses.flow_l1`` compare a flow with a reference flow.

Where the flow is valid (include/splat_hip_flow_occ.h): ``flow_attribute(depth=True)`` carries ``z2 - z1`` and ``z2`` beside
``uv2 - uv1``, ``flow_occlusion`` looks frame t2 up at ``p + flow(p)`` in one fused kernel (target outside, pixel uncovered,
something nearer at the target, forward and backward flow inconsistent) and pulls planes of frame t2 back to frame t1,
``warp_by_flow`` is the pull-back alone, ``render_flow(scene_flow=, occlusion=, cycle=)`` puts them together.  No CPU path."""
from __future__ import annotations

import ctypes
from typing import Dict, NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib as L
from .dynamics import GAUSSIAN_MAJOR, frame_table
from .frames import _Camera
from .gs.fused_ops import check_sink

SCALE_MODES = {"per_frame": L.FLOW_HEADER.defines["SPLAT_FLOW_SCALE_PER_FRAME"],
               "whole_clip": L.FLOW_HEADER.defines["SPLAT_FLOW_SCALE_WHOLE_CLIP"]}
_SCALE_GIVEN = L.FLOW_HEADER.defines["SPLAT_FLOW_SCALE_GIVEN"]
# bits of an occlusion mask (include/splat_hip_flow_occ.h)
OUTSIDE = L.FLOW_OCC_HEADER.defines["SPLAT_FLOW_OCC_OUTSIDE"]
UNCOVERED = L.FLOW_OCC_HEADER.defines["SPLAT_FLOW_OCC_UNCOVERED"]
IN_FRONT = L.FLOW_OCC_HEADER.defines["SPLAT_FLOW_OCC_IN_FRONT"]
INCONSISTENT = L.FLOW_OCC_HEADER.defines["SPLAT_FLOW_OCC_INCONSISTENT"]


# ------------------------------------------------------------------------------------------------------- flow attribute
def _cam_ref(cam: Optional[_Camera]):
    return None if cam is None else ctypes.byref(cam.struct())


def flow_attribute_forward(tab1: Tensor, tab2: Tensor, position: Tensor, pos_cubic_node: Tensor, interval_num: int,
                           cubic_layout: int, cam1: _Camera, cam2: Optional[_Camera], W: int, H: int, nearest: float = 0.01,
                           extent: float = 1.3, zero_culled: bool = False, depth: bool = False) -> Tensor:
    """raw operator (no autograd): [F, P, 2] = uv(position(tab2[f]), cam2) - uv(position(tab1[f]), cam1); ``cam2`` None: cam1.
    ``depth``: [F, P, 4] = (u2 - u1, v2 - v1, z2 - z1, z2), z the depth of the same projection (0 on a culled side)"""
    position, cubic = L.need(position, "position"), L.need(pos_cubic_node, "pos_cubic_node")
    P, F = position.shape[0], tab1.shape[0]
    if tab2.shape[0] != F:
        raise ValueError("one table entry per pair in both tables")
    if cubic.numel() != P * 4 * interval_num * 3:
        raise ValueError("pos_cubic_node must hold N * 4 * interval_num * 3 floats")
    out = torch.empty(F, P, 4 if depth else 2, dtype=torch.float32, device=position.device)
    fn = L.lib().splat_flow_attribute_depth_batch if depth else L.lib().splat_flow_attribute_batch
    L.check(fn(F, P, interval_num, L.ptr(tab1), L.ptr(tab2), L.ptr(position), L.ptr(cubic),
               cubic_layout, _cam_ref(cam1), _cam_ref(cam2), W, H, nearest, extent, 1 if zero_culled else 0, L.ptr(out), L.stream()))
    return out


def flow_attribute_backward(tab1: Tensor, tab2: Tensor, position: Tensor, pos_cubic_node: Tensor, interval_num: int,
                            cubic_layout: int, cam1: _Camera, cam2: Optional[_Camera], W: int, H: int, nearest: float,
                            extent: float, zero_culled: bool, g: Tensor, accumulate: bool, d_position: Optional[Tensor],
                            d_pos_cubic_node: Optional[Tensor]) -> None:
    """``g`` [F, P, 2] = dL/dflow (or [F, P, 4]: the gradient of the attribute with the depth) goes into ``d_position`` [P, 3]
    and ``d_pos_cubic_node`` (either may be None): stored over zero-filled buffers (``accumulate`` False) or added; one launch,
    no atomics, the same bits on every run"""
    position, cubic, g = L.need(position, "position"), L.need(pos_cubic_node, "pos_cubic_node"), L.need(g, "g")
    P, F = position.shape[0], tab1.shape[0]
    if g.dim() != 3 or tuple(g.shape[:2]) != (F, P) or g.shape[2] not in (2, 4) or tab2.shape[0] != F:
        raise ValueError(f"g must be [F={F}, P={P}, 2] (with the depth: [F, P, 4]) with one table entry per pair")
    for buf, like, name in ((d_position, position, "d_position"), (d_pos_cubic_node, cubic, "d_pos_cubic_node")):
        if buf is not None and (L.need(buf, name).numel() != like.numel() or not buf.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 buffer of the parameter's size")
    fn = L.lib().splat_flow_attribute_depth_batch_backward if g.shape[2] == 4 else L.lib().splat_flow_attribute_batch_backward
    L.check(fn(
        F, P, interval_num, L.ptr(tab1), L.ptr(tab2), L.ptr(position), L.ptr(cubic), cubic_layout, _cam_ref(cam1), _cam_ref(cam2),
        W, H, nearest, extent, 1 if zero_culled else 0, L.ptr(g), 1 if accumulate else 0, L.ptr(d_position),
        L.ptr(d_pos_cubic_node), L.stream()))


class _FlowAttribute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, position, cubic, tab1, tab2, cam1, cam2, I, layout, W, H, nearest, extent, zero_culled, sink, depth):
        out = flow_attribute_forward(tab1, tab2, position, cubic, I, layout, cam1, cam2, W, H, nearest, extent, zero_culled, depth)
        ctx.meta = (int(I), int(layout), cam1, cam2, int(W), int(H), float(nearest), float(extent), bool(zero_culled))
        ctx.sink = sink
        ctx.save_for_backward(position, cubic, tab1, tab2)
        return out

    @staticmethod
    def backward(ctx, g):
        position, cubic, tab1, tab2 = ctx.saved_tensors
        I, layout, cam1, cam2, W, H, nearest, extent, zero_culled = ctx.meta
        sink = ctx.sink or {}
        need_p, need_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        b_pos = sink.get("position") if need_p else None
        b_cub = sink.get("pos_cubic_node") if need_c else None
        r_pos = r_cub = None
        if need_p and b_pos is None:
            b_pos = r_pos = torch.zeros_like(position)
        if need_c and b_cub is None:
            b_cub = r_cub = torch.zeros_like(cubic)
        if b_pos is not None or b_cub is not None:
            flow_attribute_backward(tab1, tab2, position, cubic, I, layout, cam1, cam2, W, H, nearest, extent, zero_culled,
                                    g.contiguous(), True, b_pos, b_cub)
        return (r_pos, r_cub) + (None,) * 13


def _pair_cameras(extr, intr, extr2, intr2, F: int):
    """(cam1, cam2 or None) of F pairs: the cameras are constants, ``extr2`` / ``intr2`` default to the first camera's"""
    for t in (extr, intr, extr2, intr2):
        if isinstance(t, Tensor) and t.requires_grad:
            raise ValueError("flow_attribute: the cameras are constants (camera gradients of the flow attribute are not built); "
                             "pass them detached")
    cam1 = _Camera(extr, intr, F)
    if extr2 is None and intr2 is None:
        return cam1, None
    i2 = intr if intr2 is None else intr2
    if (intr is None) != (i2 is None):
        raise ValueError("flow_attribute: both cameras of a pair are orthographic or both pinhole")
    return cam1, _Camera(extr if extr2 is None else extr2, i2, F)


def flow_attribute(clock, times1, times2, extr: Tensor, W: int, H: int, *, position: Tensor, pos_cubic_node: Tensor,
                   intr: Optional[Tensor] = None, extr2: Optional[Tensor] = None, intr2: Optional[Tensor] = None,
                   cubic_layout: int = GAUSSIAN_MAJOR, nearest: float = 0.01, extent: float = 1.3, zero_culled: bool = False,
                   grad_sink: Optional[Dict[str, Tensor]] = None, depth: bool = False) -> Tensor:
    """[F, P, 2]: the flow of every Gaussian between the frame times ``times1[f]`` and ``times2[f]`` (fractional times
    allowed) in pixels -- ``project_point(get_position(t2)) - project_point(get_position(t1))`` -- in ONE launch each way.

    ``extr`` ([4,4] / [3,4], or one per pair [F,4,4] / [F,3,4]) and ``intr`` (None: the orthographic camera of the video
    renderer; (fx, fy, cx, cy) as [4] or [F,4]: the pinhole camera) are the camera at ``times1``; ``extr2`` / ``intr2`` the one
    at ``times2`` (None: the same camera -- the flow the frame's camera sees, the reference's case; a second camera: the flow
    of a clip taken by a moving, known camera).  A culled projection gives uv = 0 as in the reference, so a Gaussian culled at
    one time only has the attribute ``-uv1`` or ``uv2``; ``zero_culled`` writes 0 when either side is culled.  Equal times
    under one camera give exactly 0.  Differentiable w.r.t. ``position`` and ``pos_cubic_node`` (a culled side contributes
    nothing; no float atomics, bit-reproducible, allowed in deterministic mode); ``grad_sink`` as in ``positions_batch``.

    ``depth=True``: [F, P, 4] = (u2 - u1, v2 - v1, z2 - z1, z2) under the same contract; z is the depth the projection that
    gives uv returns (0 on a culled side, like uv).  Channels 0 and 1 are the bits of the two-channel attribute."""
    F = len(times1)
    if F < 1 or len(times2) != F:
        raise ValueError("flow_attribute: times1 and times2 name the two frame times of F >= 1 pairs")
    cam1, cam2 = _pair_cameras(extr, intr, extr2, intr2, F)
    sink = check_sink(grad_sink, {"position": position, "pos_cubic_node": pos_cubic_node})
    dev = position.device
    return _FlowAttribute.apply(position, pos_cubic_node, frame_table(clock, times1, dev), frame_table(clock, times2, dev),
                                cam1, cam2, int(clock.interval_num), int(cubic_layout), int(W), int(H), float(nearest),
                                float(extent), bool(zero_culled), sink, bool(depth))


# ------------------------------------------------------------------------------------------------------- flow maps
def render_flow(model, clock, times1, times2, extr: Tensor, W: int, H: int, intr: Optional[Tensor] = None,
                extr2: Optional[Tensor] = None, intr2: Optional[Tensor] = None, frames_per_batch: int = 8,
                coverage: bool = False, with_video: bool = False, differentiable: bool = False, zero_culled: bool = False,
                stats: Optional[dict] = None, nearest: float = 0.01, extent: float = 1.3, bg: float = 1.0,
                shs: Optional[Tensor] = None, cubic_layout: Optional[int] = None, capacity: Optional[int] = None,
                scene_flow: bool = False, occlusion: bool = False, cycle: bool = False, depth_margin: float = 0.05,
                min_coverage: float = 0.5, fb_alpha: float = 0.01, fb_beta: float = 0.5) -> Dict[str, Tensor]:
    """The dense optical flow of the learned video between the frame times ``times1[t]`` and ``times2[t]`` (``get_pred_flows_gs``):
    ``"flow"`` [T,2,H,W] in pixels, the flow attribute composited over the sorted lists of frame ``times1[t]`` with the opacity
    detached and background 0.  Cameras as in ``flow_attribute`` (one for the clip or one per pair).

    ``coverage``: also ``"coverage"`` [T,1,H,W], a column of ones in the same detached set (the accumulated alpha: divide a
    partly covered pixel's flow by it).  ``with_video``: also ``rgb``, ``depth`` and, when the model holds one,
    ``mask_attribute`` of frame ``times1[t]`` from the same pass (the row of ``views.render_views``).  The clip is worked through
    like ``render_views``: batches of ``frames_per_batch`` pairs, a short last batch padded with its last pair, a batch whose
    pairs outgrow the capacity rendered again (``stats``).  The attribute enters the row as a per-frame tensor: no [F,P,C] row
    is materialised.

    Forward only by default (a parameter that requires grad under grad mode raises).  ``differentiable=True``: the
    ``render_dynamic_sets(differentiable=True)`` route with ``flow_attribute`` under autograd -- gradients of the flow image
    w.r.t. the geometry of frame ``times1[t]`` (uv, conic through the parameters; the opacity is detached) and, through the
    attribute, the positions at both times: the full gradient of the reference's expression.  A frame batch holds one forward
    until its backward has run, so a differentiable clip builds one frame batch (with pair records) per batch of pairs and
    keeps them alive with the graph (``stats["frame_batch_bytes"]`` is their sum): choose ``frames_per_batch`` and the
    number of pairs with that memory in mind.

    ``scene_flow``: the detached set's row becomes ``[mask] | du dv dz z2 | [coverage]`` (``flow_attribute(depth=True)``) and
    the result gains ``"scene_flow"`` [T,1,H,W] (the composited ``z2 - z1``: with ``"flow"`` the three channels of the motion
    in camera space) and ``"track_depth"`` [T,1,H,W] (the composited ``z2``, background 0); also with ``differentiable``.
    ``occlusion`` (implies ``scene_flow`` and ``coverage``): frames ``times2`` are rendered under the second camera
    (``views.render_views``: depth on background 1, rgb) and ``flow_occlusion`` adds ``"occlusion"`` (uint8 [T,H,W], the bits
    ``OUTSIDE | UNCOVERED | IN_FRONT``), ``"depth_gap"`` [T,H,W] and ``"warped"`` [T,3,H,W], frame ``times2``'s rgb pulled back
    to frame ``times1`` (``depth_margin``, ``min_coverage`` as in ``flow_occlusion``).  ``cycle`` (needs ``occlusion``): the
    reverse flow ``times2 -> times1`` (cameras swapped) is rendered too and adds ``"fb_sq"`` [T,H,W] and the ``INCONSISTENT``
    bit (``fb_alpha``, ``fb_beta``).  The decisions are not differentiable: ``occlusion`` with ``differentiable`` raises."""
    from .layers import _params
    if cycle and not occlusion:
        raise ValueError("render_flow: cycle=True needs occlusion=True (the forward-backward test is one bit of the occlusion mask)")
    if occlusion and differentiable:
        raise ValueError("render_flow: occlusion=True is forward only (the decisions are not differentiable); render the "
                         "differentiable flow in a call of its own")
    if occlusion:
        scene_flow = coverage = True
    from .views import _GEO, _Clip, _clip_cameras, _padded, _video_sets
    times1, times2 = [float(t) for t in times1], [float(t) for t in times2]
    T = len(times1)
    if T < 1 or len(times2) != T:
        raise ValueError("render_flow: times1 and times2 name the two frame times of T >= 1 pairs")
    p, layout = _params(model, shs, cubic_layout, need_shs=with_video or occlusion)
    if not isinstance(model, dict) and "mask_attribute" not in p and isinstance(getattr(model, "mask_attribute", None), Tensor):
        p["mask_attribute"] = model.mask_attribute
    pos = p["position"]
    if not (isinstance(pos, Tensor) and pos.is_cuda):
        raise ValueError("the model must hold CUDA (ROCm) tensors (there is no CPU path)")
    # (_params detaches: the tensors the caller holds decide, and the differentiable route renders from them)
    held = {k: (model.get(k) if isinstance(model, dict) else getattr(model, k, None)) for k in _GEO}
    live = [t for t in held.values() if isinstance(t, Tensor) and t.requires_grad]
    if not differentiable and torch.is_grad_enabled() and live:
        raise ValueError("render_flow is forward only by default: call it under torch.no_grad() or with detached tensors, or "
                         "pass differentiable=True")
    P, dev = int(pos.shape[0]), pos.device
    nowhere = lambda c: torch.zeros(1, dtype=torch.float32, device=dev).expand(P, c)     # a width, no memory behind it
    # the detached set of the row: [mask_attribute] | flow (2, per frame) | [coverage]
    sets = _video_sets(p, bg) if with_video else []
    mask = sets.pop()["feature"] if len(sets) == 3 else None
    shared_head = [] if mask is None else [mask]
    shared_tail = [torch.ones(P, 1, dtype=torch.float32, device=dev)] if coverage else []
    nch = 4 if scene_flow else 2
    width = len(shared_head) + nch + len(shared_tail)
    sets.append(dict(name="flow", feature=nowhere(width), bg=0.0, detach_opacity=True))
    def new_clip(cap):
        c = _Clip(p, clock, W, H, [dict(s_) for s_ in sets], frames_per_batch, 0, nearest, extent, bg, None, layout, cap, None,
                  differentiable=bool(differentiable))
        if differentiable:
            c.geo = {k: held[k] for k in _GEO}
        return c

    clip = new_clip(capacity)
    clips = [clip]
    F = clip.F
    cams = []
    for e, i_ in ((extr, intr), (extr if extr2 is None else extr2, intr if intr2 is None else intr2)):
        e, i_ = _clip_cameras(e, i_, T, dev, "T")
        pidx = torch.tensor(_padded(T, F), device=dev)
        per_e, per_i = e.dim() == 3, i_ is not None and i_.dim() == 2
        cams.append((e.index_select(0, pidx) if per_e else e, i_.index_select(0, pidx) if per_i else i_, per_e, per_i))
    two = extr2 is not None or intr2 is not None
    cut = lambda c, b0: (c[0][b0:b0 + F] if c[2] else c[0], None if c[1] is None else (c[1][b0:b0 + F] if c[3] else c[1]))
    padded = _padded(T, F)
    parts = {k: [] for k in clip.names}
    geo = clip.geo
    for b0 in range(0, T, F):
        n = min(F, T - b0)
        t1, t2 = [times1[i] for i in padded[b0:b0 + F]], [times2[i] for i in padded[b0:b0 + F]]
        (e1, i1), (e2, i2) = cut(cams[0], b0), cut(cams[1], b0)
        with torch.set_grad_enabled(bool(differentiable) and torch.is_grad_enabled()):
            attr = flow_attribute(clock, t1, t2, e1, W, H, position=geo["position"], pos_cubic_node=geo["pos_cubic_node"], intr=i1,
                                  extr2=e2 if two else None, intr2=i2 if two else None, cubic_layout=layout, nearest=nearest,
                                  extent=extent, zero_culled=zero_culled, depth=bool(scene_flow))
        if differentiable and b0 > 0:
            # a FrameBatch holds ONE forward until its backward has run: every batch of a differentiable clip gets its own
            clip = new_clip(clip.fb.capacity)
            clips.append(clip)
        clip.sets[-1]["feature"] = shared_head + [attr] + shared_tail
        res = clip.batch(t1, e1, i1)
        for k, r in zip(clip.names, res):
            parts[k].append(r[:n])
    out = {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in parts.items()}
    row = out.pop("flow")
    c = len(shared_head)
    if mask is not None:
        out["mask_attribute"] = row[:, :1]
    out["flow"] = row[:, c:c + 2]
    if scene_flow:
        out["scene_flow"], out["track_depth"] = row[:, c + 2:c + 3], row[:, c + 3:c + 4]
    if coverage:
        out["coverage"] = row[:, c + nch:c + nch + 1]
    if stats is not None:
        stats.update(regrows=sum(c_.regrows for c_ in clips), capacity=max(c_.fb.capacity for c_ in clips),
                     frame_batch_bytes=sum(c_.fb.memory_bytes() for c_ in clips))
    if occlusion:
        from .views import render_views
        e2, i2 = (extr if extr2 is None else extr2), (intr if intr2 is None else intr2)
        common = dict(frames_per_batch=frames_per_batch, nearest=nearest, extent=extent, bg=bg, shs=shs, cubic_layout=cubic_layout)
        with torch.no_grad():
            second = render_views(model, clock, times2, e2, W, H, intr=i2, **common)       # depth on background 1
            back = None
            if cycle:      # the flow times2 -> times1: the second camera sees the start, the first the end
                back = render_flow(model, clock, times2, times1, e2, W, H, intr=i2, extr2=extr if two else None,
                                   intr2=intr if two else None, zero_culled=zero_culled, **common)["flow"]
            occ = flow_occlusion(out["flow"].contiguous(), track_depth=out["track_depth"].contiguous(),
                                 surface_depth=second["depth"], coverage=out["coverage"].contiguous(), flow_back=back,
                                 src=second["rgb"], bg_depth=1.0, depth_margin=depth_margin, min_coverage=min_coverage,
                                 fb_alpha=fb_alpha, fb_beta=fb_beta)
        out["occlusion"], out["depth_gap"], out["warped"] = occ.mask, occ.depth_gap, occ.warped
        if cycle:
            out["fb_sq"] = occ.fb_sq
    return out


# ------------------------------------------------------------------------------------------------------- occlusion, warping
class FlowOcclusion(NamedTuple):
    mask: Tensor
    depth_gap: Optional[Tensor]
    fb_sq: Optional[Tensor]
    warped: Optional[Tensor]
    counts: Optional[Tensor]


def _plane(t: Optional[Tensor], name: str) -> Optional[Tensor]:
    return None if t is None else L.need(t.detach(), name)


def _occlusion_inputs(flow, track_depth, surface_depth, coverage, flow_back, src):
    """the shape rules of ``flow_occlusion``, before any tensor is asked to live on the device"""
    if not isinstance(flow, Tensor) or flow.dim() != 4 or flow.shape[1] != 2 or min(flow.shape) < 1:
        raise ValueError("flow must be [T, 2, H, W] (u plane, v plane) with T >= 1")
    T, _, H, W = flow.shape
    if T > 65535:
        raise ValueError("flow: at most 65535 maps per call")
    if (track_depth is None) != (surface_depth is None):
        raise ValueError("track_depth and surface_depth are given both or neither (the depth test compares them)")
    for t, name in ((track_depth, "track_depth"), (surface_depth, "surface_depth"), (coverage, "coverage")):
        if t is not None and (not isinstance(t, Tensor) or tuple(t.shape) not in ((T, H, W), (T, 1, H, W))):
            raise ValueError(f"{name} must be [T, H, W] or [T, 1, H, W] with the flow's T = {T}, H = {H}, W = {W}")
    if flow_back is not None and (not isinstance(flow_back, Tensor) or flow_back.shape != flow.shape):
        raise ValueError(f"flow_back must have the flow's shape {tuple(flow.shape)}")
    if src is not None and (not isinstance(src, Tensor) or src.dim() != 4 or src.shape[0] != T or tuple(src.shape[2:]) != (H, W)
                            or not 1 <= src.shape[1] <= 8):
        raise ValueError(f"src must be [T = {T}, C, H = {H}, W = {W}] with 1 <= C <= 8 planes")
    return T, H, W


def flow_occlusion(flow: Tensor, *, track_depth: Optional[Tensor] = None, surface_depth: Optional[Tensor] = None,
                   coverage: Optional[Tensor] = None, flow_back: Optional[Tensor] = None, src: Optional[Tensor] = None,
                   bg_depth: float = 1.0, depth_margin: float = 0.05, min_coverage: float = 0.5, fb_alpha: float = 0.01,
                   fb_beta: float = 0.5, counts: bool = False) -> FlowOcclusion:
    """Where the flow ``flow`` [T,2,H,W] of frame t1 is valid, in ONE fused kernel: pixel ``p = (x, y)`` looks frame t2 up at
    ``q = p + flow(p)`` -- pixel-index coordinates: the renderer's uv carries the -0.5, pixel i's centre is index i, nothing is
    rescaled (``tracking.sample_coords`` restates a reference quirk, a ``(W - 1) / W`` rescaling, and differs) -- bilinearly,
    with the border clamped (``grid_sample(align_corners=True)`` on in-range targets).

    Returns ``(mask, depth_gap, fb_sq, warped, counts)``, None for what the inputs do not give.  ``mask`` uint8 [T,H,W]:
      ``OUTSIDE``       q is not inside [0, W-1] x [0, H-1], or the flow is not finite; nothing is sampled, the float outputs are 0
      ``UNCOVERED``     ``coverage`` [T,H,W] given and not ``coverage >= min_coverage``
      ``IN_FRONT``      ``track_depth`` (the composited z2, background 0) and ``surface_depth`` (the depth render of frame t2 on
                        background ``bg_depth``) given: ``depth_gap = td - B(surface_depth, q) > depth_margin``, something
                        nearer sits at the target; ``td = track_depth + (1 - coverage) * bg_depth`` when ``coverage`` is
                        given, so that both sides are composited over the same background
      ``INCONSISTENT``  ``flow_back`` (the flow t2 -> t1) given: ``fb_sq = |flow + B(flow_back, q)|^2 > fb_alpha (|flow|^2 +
                        |B(flow_back, q)|^2) + fb_beta`` (Sundaram et al.)
    ``IN_FRONT`` and ``INCONSISTENT`` are set only where neither ``OUTSIDE`` nor ``UNCOVERED`` is; ``depth_gap``, ``fb_sq``
    [T,H,W] and ``warped`` [T,C,H,W] (``src`` [T,C,H,W], any 1 .. 8 planes of frame t2, pulled back to frame t1) are written
    wherever not ``OUTSIDE``.  ``counts``: int32 [T,4], the pixels per bit.  Every step is one float32 operation rounded once.

    The reference's sparse test (``Tracks.occluded``) keeps its comparison ``surface >= track_depth``, which marks the points that
    are NOT hidden -- a nearer surface has the smaller depth; ``depth_gap <= 0`` is that same predicate, and the name is not
    carried over.  The defaults are a user's starting point (pixels, depth units of the scene), not tolerances.  Forward only."""
    T, H, W = _occlusion_inputs(flow, track_depth, surface_depth, coverage, flow_back, src)
    flow = L.need(flow.detach(), "flow")
    td, sd, cov = _plane(track_depth, "track_depth"), _plane(surface_depth, "surface_depth"), _plane(coverage, "coverage")
    fbk = None if flow_back is None else L.need(flow_back.detach(), "flow_back")
    src = None if src is None else L.need(src.detach(), "src")
    C = 0 if src is None else int(src.shape[1])
    dev = flow.device
    f32 = dict(dtype=torch.float32, device=dev)
    mask = torch.empty(T, H, W, dtype=torch.uint8, device=dev)
    gap = torch.empty(T, H, W, **f32) if td is not None else None
    fb = torch.empty(T, H, W, **f32) if fbk is not None else None
    warped = torch.empty(T, C, H, W, **f32) if src is not None else None
    cnt = scratch = None
    if counts:
        cnt = torch.empty(T, 4, dtype=torch.int32, device=dev)
        scratch = torch.empty(max(1, L.lib().splat_flow_occlusion_scratch_bytes(T, H, W) // 4), dtype=torch.int32, device=dev)
    L.check(L.lib().splat_flow_occlusion(T, H, W, C, L.ptr(flow), L.ptr(td), L.ptr(sd), L.ptr(cov), L.ptr(fbk), L.ptr(src),
                                         float(bg_depth), float(depth_margin), float(min_coverage), float(fb_alpha),
                                         float(fb_beta), L.ptr(mask), L.ptr(gap), L.ptr(fb), L.ptr(warped), L.ptr(cnt),
                                         L.ptr(scratch), 0 if scratch is None else scratch.numel() * 4, L.stream()))
    return FlowOcclusion(mask, gap, fb, warped, cnt)


def warp_by_flow(src: Tensor, flow: Tensor):
    """(warped [T,C,H,W], valid bool [T,H,W]): the planes ``src`` of frame t2 pulled back to frame t1 by the flow t1 -> t2 --
    ``warped(p) = B(src, p + flow(p))``, the lookup of ``flow_occlusion`` (the same kernel); ``valid`` is False where the target
    is outside the frame or the flow not finite (``warped`` is 0 there).  Forward only: the gradient of the warp is not built."""
    if src is None:
        raise ValueError("warp_by_flow: src must be [T, C, H, W]")
    occ = flow_occlusion(flow, src=src)
    return occ.warped, occ.mask == 0


# ------------------------------------------------------------------------------------------------------- colours, error
def _maps(t: Tensor, name: str) -> Tensor:
    if not isinstance(t, Tensor) or t.dim() != 4 or t.shape[1] != 2 or t.shape[0] < 1 or t.shape[2] < 1 or t.shape[3] < 1:
        raise ValueError(f"{name} must be [T, 2, H, W] (u plane, v plane) with T >= 1")
    if t.shape[0] > 65535:
        raise ValueError(f"{name}: at most 65535 maps per call")
    return L.need(t, name)


def _scratch(T: int, H: int, W: int, dev) -> Tensor:
    return torch.empty(max(1, L.lib().splat_flow_scratch_bytes(T, H, W) // 4), dtype=torch.float32, device=dev)


def flow_to_image(flow: Tensor, clip_flow: Optional[float] = None, scale="per_frame", convert_to_bgr: bool = False,
                  return_scale: bool = False):
    """uint8 [T,H,W,3]: the Middlebury colours of the flow maps ``flow`` [T,2,H,W] -- the reference's ``util.flow_to_image``
    (direction = hue on Scharstein's 55-entry wheel, radius = saturation) on the device, no host round trip.

    ``scale``: ``"per_frame"`` -- every map by its own maximum radius (the reference called on one [H,W,2] map, what the
    trainer does); ``"whole_clip"`` -- one maximum over all maps (the reference called on an [n,H,W,2] stack); a float -- that
    radius, so that several clips share one scale (the only mode in which a radius above 1, the wheel colour * 0.75, occurs).
    ``clip_flow``: clamp both components to [0, clip_flow] first (``np.clip``).  ``return_scale``: also the float32 [T] radius
    every map was divided by.  u, v, radius, angle and wheel position are float32 and the interpolation float64, as numpy
    evaluates the reference; the device's atan2 may differ from numpy's in the last bits, which moves a byte by at most one
    level where 255 * col is within rounding of an integer.  A pixel with a non-finite component is left out of the maximum
    and coloured black (the reference would spread the NaN over the whole map)."""
    flow = _maps(flow, "flow")
    T, _, H, W = flow.shape
    if isinstance(scale, str):
        if scale not in SCALE_MODES:
            raise ValueError(f"scale is one of {sorted(SCALE_MODES)} or a float radius, got {scale!r}")
        mode, given = SCALE_MODES[scale], 0.0
    else:
        mode, given = _SCALE_GIVEN, float(scale)
        if not (0.0 <= given < float("inf")):
            raise ValueError("scale must be a finite radius >= 0")
    clip = 0.0 if clip_flow is None else float(clip_flow)
    if clip_flow is not None and not clip > 0.0:
        raise ValueError("clip_flow must be positive")
    out = torch.empty(T, H, W, 3, dtype=torch.uint8, device=flow.device)
    rad = torch.empty(T, dtype=torch.float32, device=flow.device) if return_scale else None
    scratch = _scratch(T, H, W, flow.device)
    L.check(L.lib().splat_flow_to_image(T, H, W, L.ptr(flow), clip, mode, given, L.ptr(rad), L.ptr(out),
                                        1 if convert_to_bgr else 0, L.ptr(scratch), scratch.numel() * 4, L.stream()))
    return (out, rad) if return_scale else out


def flow_error_sums(pred: Tensor, gt: Tensor, weight: Optional[Tensor] = None, scale: float = 1.0, want_grad: bool = False):
    """raw operator: (sums [T,3] float64 = per map sum w (|du| + |dv|), sum w sqrt(du^2 + dv^2), sum w; grad [T,2,H,W] or None
    = scale * w * sign(d) / max(sum w, 1e-30)).  Fixed-order sums, no float atomics."""
    pred, gt = _maps(pred, "pred"), _maps(gt, "gt")
    if gt.shape != pred.shape:
        raise ValueError(f"pred and gt differ in shape: {tuple(pred.shape)} and {tuple(gt.shape)}")
    T, _, H, W = pred.shape
    if weight is not None:
        weight = L.need(weight, "weight")
        if weight.numel() != T * H * W or weight.shape[0] != T:
            raise ValueError(f"weight must be [T, H, W] or [T, 1, H, W], got {tuple(weight.shape)}")
    sums = torch.empty(T, 3, dtype=torch.float64, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    scratch = _scratch(T, H, W, pred.device)
    L.check(L.lib().splat_flow_error(T, H, W, L.ptr(pred), L.ptr(gt), L.ptr(weight), float(scale), L.ptr(sums), L.ptr(grad),
                                     L.ptr(scratch), scratch.numel() * 4, L.stream()))
    return sums, grad


@torch.no_grad()
def flow_epe(pred: Tensor, gt: Tensor, weight: Optional[Tensor] = None) -> Tensor:
    """[T] float64: the weighted mean end-point error ``sum w |pred - gt|_2 / sum w`` of every map ([T,2,H,W]; ``weight``
    [T,H,W], None: 1); a map whose weights are all zero gives 0"""
    sums, _ = flow_error_sums(pred, gt, weight)
    return sums[:, 1] / sums[:, 2].clamp_min(1e-30)
