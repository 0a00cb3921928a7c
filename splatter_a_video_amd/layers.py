"""Layer editing: render a clip from selected, moved and copied layers of ONE dynamic model (forward only).

The reference's trainer has two geometry edits by layer (src/trainer_fragGS.py): ``render_part`` (:1310-1341) renders the clip
from the Gaussians whose ``mask_attribute`` is above / not above a threshold -- object extraction / removal -- and ``add_fg``
(:1344-1405) renders the whole model plus a COPY of the foreground, evaluated at a possibly delayed time, its positions scaled
about the copy's own centroid at that time and shifted by ``delta_pos`` -- object duplication, move, resize.  Both run the model
once or twice per frame, mask / mean / ``torch.cat`` a dozen tensors and render frame by frame.

Here a *layered scene* is an ordered list of ``Layer`` s over the model.  The instances of all layers (layer by layer, inside a
layer by ascending source id: the order of the reference's ``torch.cat([base, x[fg_mask]])``) form one batch of Q instances;
per batch of frames every layer takes ONE launch of the batched dynamic preprocess reading through its instance list
(``splat_frame_preprocess_layer_batch``) with the layer's own frame table and similarity transform -- a transformed layer
one more pair of launches for its per-frame centroids (``splat_layer_centroids``) -- and binning, sort and compositing are the
frame batch's.  Features and opacity belong to the source Gaussian and are gathered per instance.

Cameras: the clip's default camera is the constructor's ``extr`` (one camera) and ``intr`` (None: orthographic; [4]: pinhole).
``render(times, extr=, intr=)`` sets the cameras of one call -- one per clip frame ([T_clip,4,4], [T_clip,4]: an orbit about the
edited scene, the two eyes of a stereo clip) or one for all -- and the layers then go through
``splat_frame_preprocess_layer_batch_cam`` (include/splat_hip_layers_cam.h).  The transform is applied in world space, so the
centroids do not depend on the camera.

Rotation: the reference sends the copy's quaternion through quaternion -> matrix -> quaternion -> normalise (:1365-1371), which
returns +-q up to rounding; the covariance does not see the sign.  Here the model's normalised rotation is used directly.
No CPU path, no gradients (the reference runs these edits under ``torch.no_grad()``)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch
from torch import Tensor

from . import _lib as L

MAX_LAYERS = 16
MAX_CHANNELS = 32


@dataclass(eq=False)        # (fields are tensors: identity, not element-wise equality)
class Layer:
    """One layer of a layered scene.

    ``select``: bool [N] (the layer's Gaussians) or None: all of them.  ``times``: None: the clip's frame times, else one time
    per clip frame for THIS layer (a delayed copy: ``max(0, t - 2)``; repeated and non-monotonic times are legal).  ``scale`` /
    ``delta`` (None, [3], or [T_clip, 3]: a per-frame drift): with ``scale != 1`` or a ``delta`` the layer is *transformed* -- its
    instances sit at ``((p - c) * scale + c) + delta_f`` in float32, ``p`` the source Gaussian's position at the layer's time of
    frame f and ``c`` the mean of exactly those ``p`` over the layer's selection (:1359-1362).  ``scale_splats``: False (the
    reference: positions only, the splats keep their size -- a shrunk copy looks denser, an enlarged one shows gaps); True also
    multiplies the activated scale by ``scale``.  An untransformed layer never goes through the transform arithmetic."""
    select: Optional[Tensor] = None
    times: Optional[Sequence[float]] = None
    scale: float = 1.0
    delta: Optional[object] = None
    scale_splats: bool = False

    def __post_init__(self):
        if self.select is not None:
            if not isinstance(self.select, Tensor):
                raise TypeError("Layer.select must be a bool tensor [N] or None")
            if self.select.dtype != torch.bool or self.select.dim() != 1:
                raise ValueError(f"Layer.select must be a bool tensor [N], got {self.select.dtype} {tuple(self.select.shape)}")
        if isinstance(self.scale, bool) or not isinstance(self.scale, (int, float)):
            raise TypeError("Layer.scale must be a float")
        self.scale = float(self.scale)
        if not math.isfinite(self.scale):
            raise ValueError("Layer.scale must be finite")
        if self.times is not None:
            self.times = [float(t) for t in self.times]
            if not all(math.isfinite(t) for t in self.times):
                raise ValueError("Layer.times must be finite")
        if self.delta is not None:
            d = torch.as_tensor(self.delta, dtype=torch.float32).detach().cpu()
            if tuple(d.shape) != (3,) and not (d.dim() == 2 and d.shape[1] == 3 and d.shape[0] >= 1):
                raise ValueError(f"Layer.delta must be [3] or [T_clip, 3], got {tuple(d.shape)}")
            if not bool(torch.isfinite(d).all()):
                raise ValueError("Layer.delta must be finite")
            self.delta = d
        self.scale_splats = bool(self.scale_splats)

    @property
    def transformed(self) -> bool:
        return self.scale != 1.0 or self.delta is not None


def foreground_mask(mask_attribute: Tensor, threshold: float = 0.5, fg: bool = True) -> Tensor:
    """bool [N]: the reference's ``mask_attribute.squeeze() > threshold`` (``fg``) or ``<= threshold`` (:1319-1322); a NaN falls
    in neither"""
    if not isinstance(mask_attribute, Tensor):
        raise TypeError("mask_attribute must be a tensor")
    m = mask_attribute.detach()
    if m.dim() == 2 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() != 1:
        raise ValueError(f"mask_attribute must be [N] or [N, 1], got {tuple(mask_attribute.shape)}")
    return (m > threshold) if fg else (m <= threshold)


def _params(model, shs, cubic_layout, need_shs: bool):
    """edit._model_params; a scene that composites explicit feature sets needs no SH coefficients"""
    from .dynamics import DynamicGaussians
    from .edit import _model_params
    has = shs is not None or (isinstance(model, dict) and isinstance(model.get("shs"), Tensor)) \
        or (isinstance(model, DynamicGaussians) and isinstance(getattr(model, "shs", None), Tensor))
    if has or need_shs:
        return _model_params(model, shs, cubic_layout)
    p, layout = _model_params(model, torch.empty(0), cubic_layout)
    p.pop("shs")
    return p, layout


def _parse_clip_sets(sets, N: int):
    if not isinstance(sets, (list, tuple)) or not sets:
        raise ValueError("sets must be a non-empty list of dicts (feature [N, c] or \"depth\", bg, detach_opacity)")
    meta, feats = [], []
    for s_ in sets:
        if not isinstance(s_, dict) or "feature" not in s_:
            raise TypeError("a set is a dict with a 'feature'")
        f = s_["feature"]
        common = (float(s_.get("bg", 0.0)), bool(s_.get("detach_opacity", False)), bool(s_.get("taps", False)))
        if isinstance(f, str):
            if f != "depth":
                raise ValueError('a set\'s feature is a tensor [N, c] or the string "depth"')
            meta.append(("depth",) + common)
            continue
        if not isinstance(f, Tensor):
            raise TypeError('a set\'s feature is a tensor [N, c] or the string "depth"')
        if f.dim() != 2 or f.shape[0] != N or f.shape[1] < 1:
            raise ValueError(f"a set's feature must be [N = {N}, c] (indexed by source Gaussian), got {tuple(f.shape)}")
        if f.dtype != torch.float32:
            raise ValueError(f"a set's feature must be float32, got {f.dtype}")
        meta.append((int(f.shape[1]),) + common)
        feats.append(f.detach())
    width = sum(1 if m[0] == "depth" else m[0] for m in meta)
    if width > MAX_CHANNELS:
        raise ValueError(f"the sets hold {width} channels, at most {MAX_CHANNELS} fit one row")
    if sum(1 for m in meta if m[3]) > 1:
        raise ValueError("at most one set feeds the densification taps")
    return meta, feats, width


def _forward_meta(meta, C):
    """Forward only, the routing groups of the one-pass plan do not change an image: when the sets as given fit no plan because
    two of them share the live-opacity group, the first live feature set takes the (unused) tap group, so that every set is
    read from its own tensor instead of a concatenated [F, Q, C] row."""
    from .frames import _one_pass_plan
    widths = [1 if m[0] == "depth" else m[0] for m in meta]
    if _one_pass_plan(meta, widths, C) is not None or any(m[3] for m in meta):
        return tuple(meta)
    for i, m in enumerate(meta):
        if m[0] != "depth" and not m[2]:
            alt = list(meta)
            alt[i] = m[:3] + (True,)
            if _one_pass_plan(tuple(alt), widths, C) is not None:
                return tuple(alt)
            break
    return tuple(meta)


def _check_clip_args(p, clock, layers, extr, W, H, sets, frames_per_batch, capacity, K, intr=None):
    """every argument check of a layered clip, on tensors of any device, before any GPU work"""
    if int(K) != 0:
        raise ValueError("LayeredClip: contributor ids (K > 0) are not built for layered scenes")
    if not isinstance(layers, (list, tuple)) or not layers:
        raise ValueError("layers must be a non-empty list of Layer")
    if len(layers) > MAX_LAYERS:
        raise ValueError(f"at most {MAX_LAYERS} layers, got {len(layers)}")
    if not all(isinstance(l_, Layer) for l_ in layers):
        raise TypeError("layers must be a list of Layer")
    if int(W) < 1 or int(H) < 1:
        raise ValueError("W and H must be positive")
    if isinstance(frames_per_batch, bool) or int(frames_per_batch) != frames_per_batch or not (1 <= int(frames_per_batch) <= 65535):
        raise ValueError("frames_per_batch must be an integer in 1 .. 65535")
    if capacity is not None and int(capacity) < 1:
        raise ValueError("capacity must be positive")
    pos = p["position"]
    if not isinstance(pos, Tensor) or pos.dim() != 2 or pos.shape[1] != 3 or pos.shape[0] < 1:
        raise ValueError("model position must be [N, 3]")
    N, I = int(pos.shape[0]), int(clock.interval_num)
    want = dict(pos_cubic_node=N * 4 * I * 3, rotation=N * 4, rot_poly_feat=N * 16, rot_fourier_feat=N * 32, opacity=N,
                scaling=N * 3)
    for k, n in want.items():
        if not isinstance(p[k], Tensor) or p[k].numel() != n:
            raise ValueError(f"model {k} does not hold {n} values (N = {N} Gaussians, {I} spline segments)")
    if not isinstance(extr, Tensor) or tuple(extr.shape) not in ((4, 4), (3, 4)):
        raise ValueError("extr must be one camera, [4, 4] or [3, 4]")
    if intr is not None and (not isinstance(intr, Tensor) or intr.dtype != torch.float32 or tuple(intr.shape) != (4,)):
        raise ValueError("intr must be None or one pinhole camera, float32 (fx, fy, cx, cy) [4] (per-frame cameras: render(...))")
    for li, l_ in enumerate(layers):
        if l_.select is not None:
            if l_.select.shape[0] != N:
                raise ValueError(f"layer {li}: select must be [N = {N}], got {tuple(l_.select.shape)}")
            if not bool(l_.select.any()):
                raise ValueError(f"layer {li}: the selection is empty")
    meta, feats, C = _parse_clip_sets(sets, N)
    return N, I, meta, feats, C


def clip_layer_inputs(layers: Sequence[Layer], times):
    """the clip's frame times and, per layer, the layer's time of every clip frame and its per-frame delta [T_clip, 3] (None:
    none); checks the layers' time lists and per-frame deltas against the clip's length (no GPU work)"""
    times = [float(t) for t in times]
    T = len(times)
    if T < 1:
        raise ValueError("a clip needs at least one frame time")
    lt, ld = [], []
    for li, l_ in enumerate(layers):
        if l_.times is not None and len(l_.times) != T:
            raise ValueError(f"layer {li}: {len(l_.times)} times for a clip of {T} frames")
        lt.append(times if l_.times is None else l_.times)
        d = l_.delta
        if d is not None:
            if d.dim() == 2 and d.shape[0] != T:
                raise ValueError(f"layer {li}: delta must be [3] or [T_clip = {T}, 3], got {tuple(d.shape)}")
            d = d.reshape(1, 3).expand(T, 3) if d.dim() == 1 else d
        ld.append(d)
    return times, lt, ld


class LayeredClip:
    """A clip rendered from the layers ``layers`` of ``model`` (a parameter dict or a ``DynamicGaussians``, as
    ``tracking.track_pixels`` and ``edit.fit_appearance`` take it) under the clip's default camera: ``extr`` ([4,4] / [3,4], one
    camera) and ``intr`` (None: the orthographic video camera; (fx, fy, cx, cy) [4]: the pinhole camera).

    ``sets``: the feature sets of ``FrameBatch.render_dynamic_sets`` (dicts ``feature`` [N, c] or ``"depth"``, ``bg``,
    ``detach_opacity``), features indexed by SOURCE Gaussian; ``"depth"`` is the instance's own projected depth.  The constructor
    builds the instance list, gathers the features per instance once and owns one ``FrameBatch(frames_per_batch, Q, W, H, C)``.
    ``render(times, extr=None, intr=None)`` returns one image tensor [T_clip, c, H, W] per set, under the default camera or the
    cameras of that call.  Contributor ids (``K > 0``) are not built."""

    def __init__(self, model, clock, layers: Sequence[Layer], extr: Tensor, W: int, H: int, sets, frames_per_batch: int = 8,
                 shs: Optional[Tensor] = None, cubic_layout: Optional[int] = None, nearest: float = 0.01, extent: float = 1.3,
                 capacity: Optional[int] = None, K: int = 0, intr: Optional[Tensor] = None):
        p, layout = _params(model, shs, cubic_layout, need_shs=False)
        N, I, meta, feats, C = _check_clip_args(p, clock, layers, extr, W, H, sets, frames_per_batch, capacity, K, intr)
        pos = p["position"]
        dev = pos.device
        if dev.type != "cuda":
            raise ValueError("LayeredClip lives on the GPU: the model must hold CUDA (ROCm) tensors (there is no CPU path)")
        from .frames import FrameBatch
        from .gs.point_ops import _extr12
        self.clock, self.layers, self.layout = clock, list(layers), layout
        self.N, self.I, self.W, self.H, self.C = N, I, int(W), int(H), C
        self.F = int(frames_per_batch)
        self.nearest, self.extent = float(nearest), float(extent)
        self.p = {k: L.need(p[k], k) for k in ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat",
                                                "opacity", "scaling")}
        self.extr = _extr12(extr.detach())
        # the default camera as ``render`` takes one: None without ``intr`` (the one orthographic camera: today's launches)
        self.camera = None if intr is None else (extr.detach().to(dev).contiguous(), intr.detach().to(dev).contiguous())
        # the instance list: layer by layer, ascending source ids inside a layer
        self.src: List[Optional[Tensor]] = []
        self.q0: List[int] = []
        self.S: List[int] = []
        q = 0
        for l_ in self.layers:
            ids = None if l_.select is None else torch.nonzero(l_.select.to(dev), as_tuple=False)[:, 0].to(torch.int32).contiguous()
            self.src.append(ids)
            self.q0.append(q)
            self.S.append(N if ids is None else int(ids.numel()))
            q += self.S[-1]
        if q > 0x7fffffff:
            raise ValueError("too many instances")
        self.Q = q
        if len(self.layers) == 1 and self.src[0] is None:
            self.feats = [L.need(f, "feature") for f in feats]
        else:
            every = torch.arange(N, dtype=torch.int64, device=dev)
            gather = torch.cat([every if ids is None else ids.to(torch.int64) for ids in self.src])
            self.feats = [L.need(f, "feature").index_select(0, gather) for f in feats]
        self.meta = _forward_meta(meta, C)
        self.widths = [1 if m[0] == "depth" else m[0] for m in self.meta]
        self.fb = FrameBatch(self.F, self.Q, self.W, self.H, C, dev, capacity=capacity, records=False)    # forward only
        self.opa_t = torch.empty(self.Q, 1, dtype=torch.float32, device=dev)
        lib = L.lib()
        self._centroid = {li: torch.empty(self.F, 3, dtype=torch.float32, device=dev)
                          for li, l_ in enumerate(self.layers) if l_.transformed}
        nbytes = max([int(lib.splat_layer_centroids_scratch_bytes(self.F, self.S[li])) for li in self._centroid] + [8])
        self._scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        self._tables: Dict[tuple, Tensor] = {}
        self.table_builds = 0       # frame tables built so far (a later render of the same times builds none)
        self.regrows = 0            # batches rendered again after their pairs outgrew the capacity

    # ------------------------------------------------------------------
    def _table(self, times: tuple) -> Tensor:
        tab = self._tables.get(times)
        if tab is None:
            from .dynamics import frame_table
            tab = frame_table(self.clock, list(times), self.fb.dev)
            self._tables[times] = tab
            self.table_builds += 1
        return tab

    @torch.no_grad()
    def render(self, times: Sequence[float], extr: Optional[Tensor] = None, intr: Optional[Tensor] = None) -> List[Tensor]:
        """the clip at the frame times ``times``: one detached image tensor [T_clip, c, H, W] per set.  The clip is worked through
        in batches of ``frames_per_batch`` frames (a short last batch is padded with its last frame, the padding dropped).  A
        batch whose tile-Gaussian pairs outgrow the pair capacity is never returned: the capacity is raised and the batch
        rendered again (one host synchronisation per batch reads the pair counts).

        ``extr`` / ``intr``: the cameras of this call in place of the clip's default camera -- ``extr`` [4,4] / [3,4] or one per
        clip frame [T_clip,4,4] / [T_clip,3,4]; ``intr`` None (orthographic), (fx, fy, cx, cy) [4] or [T_clip,4] (pinhole).  An
        ``extr`` alone keeps the default ``intr``, an ``intr`` alone the default ``extr``.  A ``"depth"`` set is the instance's
        depth under its frame's camera.  Without either, a clip built without ``intr`` issues the launches of the one
        orthographic camera."""
        times, lt, ld = clip_layer_inputs(self.layers, times)
        T = len(times)
        F, dev = self.F, self.fb.dev
        from .views import _batch_cameras, _padded
        padded = _padded(T, F)
        cams = _batch_cameras(extr, intr, self.camera or (self.extr, None), T, F, dev, "T_clip")
        deltas = [None if d is None else d[padded].contiguous().to(dev) for d in ld]
        outs = [torch.empty(T, w, self.H, self.W, dtype=torch.float32, device=dev) for w in self.widths]
        for b0 in range(0, T, F):
            idx = padded[b0:b0 + F]
            n = min(F, T - b0)
            row = self._render_batch([tuple(t_[i] for i in idx) for t_ in lt], [None if d is None else d[b0:b0 + F] for d in deltas],
                                     None if cams is None else cams[b0 // F])
            c0 = 0
            for o, w in zip(outs, self.widths):
                o[b0:b0 + n].copy_(row[:n, c0:c0 + w])
                c0 += w
        return outs

    def _render_batch(self, layer_times, layer_deltas, cam=None) -> Tensor:
        from .frames import _blend_sets_forward, _entry
        fb, lib, st, p = self.fb, L.lib(), L.stream(), self.p
        F = self.F
        fb._begin_forward()
        for li, l_ in enumerate(self.layers):
            tab = self._table(layer_times[li])
            cen = None
            if l_.transformed:
                cen = self._centroid[li]
                L.check(lib.splat_layer_centroids(
                    F, self.N, self.S[li], self.I, L.ptr(tab), L.ptr(self.src[li]), L.ptr(p["position"]),
                    L.ptr(p["pos_cubic_node"]), self.layout, L.ptr(cen), L.ptr(self._scratch),
                    self._scratch.numel() * 8, st))
            pre, cam_arg = _entry("splat_frame_preprocess_layer_batch", cam, self.extr)
            L.check(pre(
                F, self.N, self.S[li], self.Q, self.q0[li], self.I, L.ptr(tab),
                L.ptr(self.src[li]), L.ptr(p["position"]), L.ptr(p["pos_cubic_node"]), self.layout, L.ptr(p["rotation"]),
                L.ptr(p["rot_poly_feat"]), L.ptr(p["rot_fourier_feat"]), L.ptr(p["opacity"]), L.ptr(p["scaling"]), cam_arg,
                self.W, self.H, self.nearest, self.extent, L.ptr(cen), L.ptr(layer_deltas[li]),
                l_.scale, 1 if l_.scale_splats else 0, L.ptr(fb.uv), L.ptr(fb.depth), L.ptr(fb.conic), L.ptr(fb.radius),
                L.ptr(self.opa_t), st))
        # the sort drops surplus pairs: no image is composited from lists that did not fit (one synchronisation per batch)
        self.regrows += fb._bin_and_sort_fitting(self.opa_t)
        out, _, _ = _blend_sets_forward(fb, self.meta, self.feats, self.opa_t, 0, 0)
        return out


def _wrapper_model(model, shs, cubic_layout, mask_attribute):
    p, layout = _params(model, shs, cubic_layout, need_shs=True)
    N = int(p["position"].shape[0]) if isinstance(p["position"], Tensor) and p["position"].dim() == 2 else -1
    if not isinstance(p["shs"], Tensor) or p["shs"].dim() != 3 or tuple(p["shs"].shape) != (N, 16, 3):
        raise ValueError(f"shs must be [N = {N}, 16, 3]")
    m = mask_attribute if mask_attribute is not None else (model.get("mask_attribute") if isinstance(model, dict)
                                                           else getattr(model, "mask_attribute", None))
    if not isinstance(m, Tensor):
        raise ValueError("no mask: the model holds no 'mask_attribute'; pass mask_attribute=")
    m = m.detach()
    if tuple(m.shape) not in ((N,), (N, 1)):
        raise ValueError(f"mask_attribute must be [N = {N}] or [N, 1], got {tuple(m.shape)}")
    if m.dtype != torch.float32:
        raise ValueError(f"mask_attribute must be float32, got {m.dtype}")
    return p, layout, m.reshape(N, 1)


def _colors(shs: Tensor) -> Tensor:
    if not shs.is_cuda:
        raise ValueError("the model must hold CUDA (ROCm) tensors (there is no CPU path)")
    from .renderer import OrthoEnhancedRenderer
    return OrthoEnhancedRenderer.colors(L.need(shs, "shs")).detach()


def _edit_sets(rgb, mask, bg):
    """the reference's blends of an edit: rgb | depth (bg 1) | mask_attribute with opacity.detach() (render_iter)"""
    return [dict(feature=rgb, bg=float(bg), taps=True), dict(feature="depth", bg=1.0),
            dict(feature=mask, bg=0.0, detach_opacity=True)]


def _edit_clip(p, layout, m, clock, layers, times, extr, W, H, bg, frames_per_batch, nearest, extent, capacity, intr=None
               ) -> Dict[str, Tensor]:
    # every argument check first (the DC rows stand in for the colours: a view, no launch), then the colours, then the clip
    per_frame = isinstance(extr, Tensor) and extr.dim() == 3 and extr.shape[0] >= 1
    one = extr[0] if per_frame else extr        # the clip's default camera is one camera; the call's cameras go to render()
    _check_clip_args(p, clock, layers, one, W, H, _edit_sets(p["shs"][:, 0, :], m, bg), frames_per_batch, capacity, 0)
    ts, _, _ = clip_layer_inputs(layers, times)
    if per_frame or intr is not None:
        from .views import _clip_cameras
        _clip_cameras(extr, intr, len(ts), extr.device, "T")
    clip = LayeredClip(p, clock, layers, one, W, H, _edit_sets(_colors(p["shs"]), m, bg), frames_per_batch, cubic_layout=layout,
                       nearest=nearest, extent=extent, capacity=capacity)
    images = clip.render(times, extr, intr) if (per_frame or intr is not None) else clip.render(times)
    return dict(zip(("rgb", "depth", "mask_attribute"), images))


def render_part(model, clock, times, extr: Tensor, W: int, H: int, fg: bool = True, threshold: float = 0.5, bg: float = 1.0,
                mask_attribute: Optional[Tensor] = None, shs: Optional[Tensor] = None, cubic_layout: Optional[int] = None,
                frames_per_batch: int = 8, nearest: float = 0.01, extent: float = 1.3, capacity: Optional[int] = None,
                intr: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """The reference's ``render_part`` (:1310-1341): the clip from only the Gaussians whose ``mask_attribute`` is above (``fg``)
    or not above ``threshold`` -- a foreground-only or background-only video on the background colour ``bg`` (the reference: 1).
    Colours from the SH coefficients (``model["shs"]`` or ``shs=``), the mask from ``model["mask_attribute"]`` or
    ``mask_attribute=``.  ``extr`` one camera or one per frame time [T,4,4]; ``intr`` None, [4] or [T,4]: the pinhole camera (as
    ``LayeredClip.render`` takes them).  Returns ``rgb`` [T, 3, H, W], ``depth`` and ``mask_attribute`` [T, 1, H, W]."""
    p, layout, m = _wrapper_model(model, shs, cubic_layout, mask_attribute)
    sel = foreground_mask(m, threshold, fg)
    if not bool(sel.any()):
        raise ValueError("render_part: the selection is empty")
    return _edit_clip(p, layout, m, clock, [Layer(select=sel)], times, extr, W, H, bg, frames_per_batch, nearest, extent, capacity,
                      intr)


def add_foreground(model, clock, times, extr: Tensor, W: int, H: int, delta, scale: float, fg_threshold: float = 0.5,
                   delay: float = 0, drift=None, bg: float = 0.0, scale_splats: bool = False,
                   mask_attribute: Optional[Tensor] = None, shs: Optional[Tensor] = None, cubic_layout: Optional[int] = None,
                   frames_per_batch: int = 8, nearest: float = 0.01, extent: float = 1.3, capacity: Optional[int] = None,
                   intr: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """The reference's ``add_fg`` (:1344-1405): every frame from the whole model plus a copy of the foreground
    (``mask_attribute > fg_threshold``) evaluated at ``max(0, t - delay)`` (the reference's commented "for cow" line: 2), scaled
    by ``scale`` about the copy's centroid at that time and shifted by ``delta + drift * max(0, t - delay)`` ([3] each; the
    reference's per-frame drift of ``delta_pos``).  ``extr`` / ``intr``: cameras as in ``render_part``.  Returns ``rgb``, ``depth``
    and ``mask_attribute`` images as ``render_part``."""
    p, layout, m = _wrapper_model(model, shs, cubic_layout, mask_attribute)
    times = [float(t) for t in times]
    if not math.isfinite(float(delay)) or float(delay) < 0:
        raise ValueError("delay must be >= 0")
    d = torch.as_tensor(delta, dtype=torch.float32).detach().cpu()
    if tuple(d.shape) not in ((3,), (1, 3)):
        raise ValueError(f"delta must be [3], got {tuple(d.shape)}")
    d = d.reshape(3)
    ltimes = [max(0.0, t - float(delay)) for t in times]
    if drift is not None:
        dr = torch.as_tensor(drift, dtype=torch.float32).detach().cpu()
        if tuple(dr.shape) not in ((3,), (1, 3)):
            raise ValueError(f"drift must be [3], got {tuple(dr.shape)}")
        d = d.reshape(1, 3) + dr.reshape(1, 3) * torch.tensor(ltimes, dtype=torch.float32).reshape(-1, 1)
    sel = foreground_mask(m, fg_threshold, True)
    if not bool(sel.any()):
        raise ValueError("add_foreground: the foreground selection is empty")
    layers = [Layer(), Layer(select=sel, times=ltimes, scale=scale, delta=d, scale_splats=scale_splats)]
    return _edit_clip(p, layout, m, clock, layers, times, extr, W, H, bg, frames_per_batch, nearest, extent, capacity, intr)
