"""Feature lifting: per-Gaussian features from per-frame 2-D maps (DINO / SAM features, a painted mask, any per-pixel signal).

The reference can only render a per-Gaussian feature field; its feature losses are dead code (src/trainer_fragGS.py:631-642,
``mask_attribute`` / ``dino_attribute`` under ``if False``) and "consistent feature generation" is an open TODO of its README.
With geometry and opacity frozen the composited image is linear in the feature, ``out[p, c] = sum_g w[p, g] f[g, c]`` with
``w = alpha * T`` under the forward's skip and stop rules, so a feature fit needs the transposed operator alone:

    num[g, c] = sum_frames sum_p pw[p] w[p, g] y[p, c]        den[g] = sum_frames sum_p pw[p] w[p, g]

``num / den`` is the visibility-weighted average of what Gaussian g shows over the clip (the one-pass lift, ``FeatureLift.add`` /
``lift_features``), and ``A^T (pw (A f - y))`` is the exact gradient of the least-squares fit (``FeatureLift.refine``).  Per batch of
frames: the dynamic preprocess, binning and sort of a ``FrameBatch``, then per chunk of 32 channels splat_blend_lift_batch (one
launch over (frame, tile): a front-to-back walk, no replay, no dL/dalpha, no geometry terms) and splat_lift_fold (one streaming
launch).  No float atomics anywhere: two lifts of the same inputs give the same bits, with ``splat_set_deterministic(1)`` or
without.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib as L

CHUNK = 32          # channels per launch (the record of a list entry holds at most 32 sums and the weight sum)


def _chunks(D: int):
    """(c0, cn, want_den) per launch: the weight sum rides with the last chunk, the narrowest"""
    cs = [(c0, min(CHUNK, D - c0)) for c0 in range(0, D, CHUNK)]
    return [(c0, cn, k == len(cs) - 1) for k, (c0, cn) in enumerate(cs)]


def _check_maps(maps, pixel_weight, F: Optional[int], D: Optional[int], W: int, H: int) -> Tuple[int, int]:
    """shape and dtype checks on tensors of any device; returns (F, D)"""
    if not isinstance(maps, Tensor):
        raise TypeError("maps must be a torch.Tensor")
    want = f"[{'F' if F is None else F}, {'D' if D is None else D}, H = {H}, W = {W}]"
    if maps.dim() != 4 or maps.shape[0] < 1 or maps.shape[1] < 1 or tuple(maps.shape[2:]) != (H, W) \
            or (F is not None and maps.shape[0] != F) or (D is not None and maps.shape[1] != D):
        raise ValueError(f"maps must have shape [F, D, H, W] = {want}, got {tuple(maps.shape)}")
    if maps.dtype != torch.float32:
        raise ValueError(f"maps must be float32, got {maps.dtype}")
    F, D = int(maps.shape[0]), int(maps.shape[1])
    if pixel_weight is not None:
        if not isinstance(pixel_weight, Tensor):
            raise TypeError("pixel_weight must be a torch.Tensor or None")
        if tuple(pixel_weight.shape) != (F, H, W):
            raise ValueError(f"pixel_weight must have shape [F, H, W] = {(F, H, W)}, got {tuple(pixel_weight.shape)}")
        if pixel_weight.dtype != torch.float32:
            raise ValueError(f"pixel_weight must be float32, got {pixel_weight.dtype}")
    return F, D


def _lift_chunks(F, P, D, uv, conic, opacity, op_fs, idx_sorted, tile_range, slot_sorted, goff, cap, W, H, maps, pixel_weight, rec,
                 num, den) -> None:
    """the two launches per chunk of 32 channels; ``den`` None: no weight sum"""
    lib, st = L.lib(), L.stream()
    for c0, cn, last in _chunks(D):
        wd = 1 if (last and den is not None) else 0
        L.check(lib.splat_blend_lift_batch(
            F, P, D, c0, cn, L.ptr(uv), L.ptr(conic), L.ptr(opacity), op_fs,
            L.ptr(idx_sorted), L.ptr(tile_range), L.ptr(slot_sorted), cap, W, H, L.ptr(maps),
            L.ptr(pixel_weight), wd, L.ptr(rec), st))
        L.check(lib.splat_lift_fold(F, P, cn, wd, cap, L.ptr(goff), L.ptr(rec), L.ptr(num),
                                    D, c0, L.ptr(den if wd else None), st))


def _record_floats(D: int) -> int:
    return int(L.lib().splat_lift_pair_stride(min(D, CHUNK), 1))


@torch.no_grad()
def blend_lift(uv: Tensor, conic: Tensor, opacity: Tensor, idx_sorted: Tensor, tile_range: Tensor, pairmap, maps: Tensor, W: int,
               H: int, pixel_weight: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(num [P, D], den [P]) of ONE frame's sorted lists (``gs.sort_gaussian`` / ``sort_gaussian_capped`` with their pair map):
    ``num[g, c] = sum_p pw[p] w[p, g] maps[c, p]``, ``den[g] = sum_p pw[p] w[p, g]`` with the weights ``w = alpha * T`` of
    ``gs.alpha_blending`` on the same lists.  ``maps`` [D, H, W] (or [1, D, H, W]), any D >= 1, worked through in chunks of 32
    channels; ``pixel_weight`` [H, W] (or [1, H, W]); a pixel of weight 0 contributes exactly 0 whatever its map value."""
    W, H = int(W), int(H)
    if W < 1 or H < 1:
        raise ValueError("W and H must be >= 1")
    for name, t in (("uv", uv), ("conic", conic), ("opacity", opacity), ("idx_sorted", idx_sorted), ("tile_range", tile_range)):
        if not isinstance(t, Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    P = int(opacity.numel())
    if P < 1 or uv.numel() != 2 * P or conic.numel() != 3 * P:
        raise ValueError("uv [P,2] / conic [P,3] / opacity [P] must agree on P >= 1")
    T = ((W + 15) // 16) * ((H + 15) // 16)
    if tile_range.numel() != 2 * T:
        raise ValueError("tile_range must have shape [ceil(W/16)*ceil(H/16), 2]")
    if isinstance(maps, Tensor) and maps.dim() == 3:
        maps = maps[None]
    if isinstance(pixel_weight, Tensor) and pixel_weight.dim() == 2:
        pixel_weight = pixel_weight[None]
    _, D = _check_maps(maps, pixel_weight, 1, None, W, H)
    if pairmap is None or not hasattr(pairmap, "goff") or not hasattr(pairmap, "slot_sorted"):
        raise ValueError("pairmap must be the pair map of the sort that made idx_sorted (status.pairmap)")
    uv, conic, opacity = L.need(uv.detach(), "uv"), L.need(conic.detach(), "conic"), L.need(opacity.detach(), "opacity")
    idx_sorted, tile_range = L.need(idx_sorted, "idx_sorted", torch.int32), L.need(tile_range, "tile_range", torch.int32)
    maps = L.need(maps.detach(), "maps")
    pixel_weight = None if pixel_weight is None else L.need(pixel_weight.detach(), "pixel_weight")
    goff, slot_sorted = L.need(pairmap.goff, "pairmap.goff", torch.int32), L.need(pairmap.slot_sorted, "pairmap.slot_sorted", torch.int32)
    M = int(idx_sorted.numel())
    if goff.numel() != P or slot_sorted.numel() != M:
        raise ValueError("the pair map does not belong to these lists (goff [P], slot_sorted [M])")
    num = torch.zeros(P, D, dtype=torch.float32, device=uv.device)
    den = torch.zeros(P, dtype=torch.float32, device=uv.device)
    if M == 0:
        return num, den
    rec = torch.empty(M * _record_floats(D), dtype=torch.float32, device=uv.device)
    _lift_chunks(1, P, D, uv, conic, opacity, 0, idx_sorted, tile_range, slot_sorted, goff, M, W, H, maps, pixel_weight, rec, num, den)
    return num, den


class FeatureLift:
    """Per-Gaussian features of a dynamic model from per-frame maps.

    ``model``: a parameter dict (position, pos_cubic_node, rotation, rot_poly_feat, rot_fourier_feat, opacity (logit), scaling
    (log)) or a ``DynamicGaussians``, as ``edit.fit_appearance`` and ``layers.LayeredClip`` take it; ``extr`` ([4, 4] / [3, 4], one
    camera) and ``intr`` (None: the orthographic video camera; (fx, fy, cx, cy) [4]: the pinhole camera) the default camera;
    ``D`` the width of the maps.  ``add`` / ``gradient`` / ``refine`` take ``extr=`` / ``intr=`` for the cameras the call's frames
    were taken by: one for all, or one per frame time ([T,4,4] / [T,3,4], [T,4] -- a video from a moving, known camera); they
    then go through ``splat_frame_preprocess_layer_batch_cam`` (include/splat_hip_layers_cam.h).  The object holds ONE ``FrameBatch`` of ``frames_per_batch`` frames for
    geometry, binning and sort (the batch's composited row is never used) and the sums ``num`` [N, D] / ``den`` [N].

    ``add(times, maps, pixel_weight=None)`` accumulates over any number of calls; ``result()`` returns
    ``(feature [N, D] = where(den > 0, num / den, 0), weight [N] = den)``; ``refine`` runs the least-squares fit from a start."""

    def __init__(self, model, clock, extr: Tensor, W: int, H: int, D: int, frames_per_batch: int = 8, capacity: Optional[int] = None,
                 cubic_layout: Optional[int] = None, nearest: float = 0.01, extent: float = 1.3, intr: Optional[Tensor] = None):
        from .layers import _params
        from .tracking import _NAMES, _cull_args
        p, layout = _params(model, None, cubic_layout, need_shs=False)
        W, H, D = int(W), int(H), int(D)
        if W < 1 or H < 1:
            raise ValueError("W and H must be >= 1")
        if D < 1:
            raise ValueError("D must be >= 1")
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
            raise ValueError("intr must be None or one pinhole camera, float32 (fx, fy, cx, cy) [4] (per-frame cameras: add(...))")
        src = model if isinstance(model, dict) else {k: getattr(model, k) for k in _NAMES}
        self.model_requires_grad = any(isinstance(src.get(k), Tensor) and src[k].requires_grad for k in _NAMES)
        dev = pos.device
        if dev.type != "cuda":
            raise ValueError("FeatureLift lives on the GPU: the model must hold CUDA (ROCm) tensors (there is no CPU path)")
        from .frames import FrameBatch
        from .gs.point_ops import _extr12
        self.clock, self.layout = clock, layout
        self.N, self.I, self.W, self.H, self.D, self.F = N, I, W, H, D, int(frames_per_batch)
        self.nearest, self.extent = _cull_args(nearest, extent)
        self.p = {k: L.need(p[k], k) for k in _NAMES}
        self.extr = _extr12(extr.detach())
        # the default camera as a call takes one: None without ``intr`` (the one orthographic camera: the core entry point)
        self.camera = None if intr is None else (extr.detach().to(dev).contiguous(), intr.detach().to(dev).contiguous())
        self.fb = FrameBatch(self.F, N, W, H, 1, dev, capacity=None if capacity is None else int(capacity),
                             records=False)     # forward only: the lift keeps its own ("lift", "rec") records
        self.opa_t = torch.empty(N, 1, dtype=torch.float32, device=dev)
        self.num = torch.zeros(N, D, dtype=torch.float32, device=dev)
        self.den = torch.zeros(N, dtype=torch.float32, device=dev)
        self._tables = {}
        self.regrows = 0            # batches binned again after their pairs outgrew the capacity

    # ------------------------------------------------------------------
    def _batches(self, times: Sequence[float], cams=None):
        """(first frame, frames, the batch's F frame times: a short last batch repeats its last frame, the batch's ``_Camera``
        -- None without ``cams``, the result of ``_cameras``)"""
        times = [float(t) for t in times]
        T, F = len(times), self.F
        for b0 in range(0, T, F):
            yield b0, min(F, T - b0), tuple(times[min(b0 + i, T - 1)] for i in range(F)), None if cams is None else cams[b0 // F]

    def _cameras(self, T: int, extr, intr):
        """the ``_Camera`` of every batch of a call over T frame times (``views._batch_cameras``); None for the one orthographic
        camera of the constructor"""
        from .views import _batch_cameras
        return _batch_cameras(extr, intr, self.camera or (self.extr, None), T, self.F, self.fb.dev, "T")

    def _geometry(self, times: tuple, checked: bool, cam=None) -> None:
        """the batch's preprocess, binning and sort.  ``checked``: a batch whose tile-Gaussian pairs outgrow the pair capacity
        is binned again with a larger one -- nothing is ever folded in from truncated lists (one host synchronisation per batch
        reads the pair counts).  ``cam``: the batch's ``_Camera``; None: the one orthographic camera of the constructor"""
        from .dynamics import frame_table
        from .frames import _entry
        fb, st, p = self.fb, L.stream(), self.p
        tab = self._tables.get(times)
        if tab is None:
            tab = self._tables[times] = frame_table(self.clock, list(times), fb.dev)
        fb._begin_forward()
        pre, cam_arg = _entry("splat_frame_preprocess_layer_batch", cam, self.extr)
        L.check(pre(
            self.F, self.N, self.N, self.N, 0, self.I, L.ptr(tab), L.ptr(None),
            L.ptr(p["position"]), L.ptr(p["pos_cubic_node"]), self.layout, L.ptr(p["rotation"]), L.ptr(p["rot_poly_feat"]),
            L.ptr(p["rot_fourier_feat"]), L.ptr(p["opacity"]), L.ptr(p["scaling"]), cam_arg, self.W, self.H,
            self.nearest, self.extent, L.ptr(None), L.ptr(None), 1.0, 0, L.ptr(fb.uv), L.ptr(fb.depth),
            L.ptr(fb.conic), L.ptr(fb.radius), L.ptr(self.opa_t), st))
        self.regrows += fb._bin_and_sort_fitting(self.opa_t, checked)

    def _records(self) -> Tensor:
        return self.fb._set_buffer(("lift", "rec"), self.F * self.fb.capacity * _record_floats(self.D))

    def _lift(self, n: int, maps: Tensor, pixel_weight: Optional[Tensor], num: Tensor, den: Optional[Tensor]) -> None:
        fb = self.fb
        _lift_chunks(n, self.N, self.D, fb.uv, fb.conic, self.opa_t, 0, fb.idx_sorted, fb.tile_range, fb.slot_sorted, fb.goff,
                     fb.capacity, self.W, self.H, maps, pixel_weight, self._records(), num, den)

    def _inputs(self, times, maps, pixel_weight):
        times = list(times)
        if not times:
            raise ValueError("times holds no frame")
        _check_maps(maps, pixel_weight, len(times), self.D, self.W, self.H)
        maps = L.need(maps.detach(), "maps")
        pixel_weight = None if pixel_weight is None else L.need(pixel_weight.detach(), "pixel_weight")
        return times, maps, pixel_weight

    @torch.no_grad()
    def add(self, times: Sequence[float], maps: Tensor, pixel_weight: Optional[Tensor] = None, extr: Optional[Tensor] = None,
            intr: Optional[Tensor] = None) -> "FeatureLift":
        """accumulate ``num`` / ``den`` over the frames ``times`` with the maps ``maps`` [F, D, H, W] (``pixel_weight`` [F, H, W]);
        ``extr`` / ``intr``: the cameras the frames were taken by (one, or one per frame time) in place of the default camera"""
        times, maps, pixel_weight = self._inputs(times, maps, pixel_weight)
        cams = self._cameras(len(times), extr, intr)
        for b0, n, bt, cam in self._batches(times, cams):
            self._geometry(bt, checked=True, cam=cam)
            self._lift(n, maps[b0:b0 + n], None if pixel_weight is None else pixel_weight[b0:b0 + n], self.num, self.den)
        return self

    def result(self) -> Tuple[Tensor, Tensor]:
        """(feature [N, D], weight [N]): an unseen Gaussian (weight 0) gets 0, never NaN"""
        seen = (self.den > 0)[:, None]
        feature = torch.where(seen, self.num / torch.where(seen, self.den[:, None], torch.ones_like(self.den[:, None])),
                              torch.zeros_like(self.num))
        return feature, self.den.clone()

    # ------------------------------------------------------------------ least squares from a start
    def _forward(self, n: int, feature: Tensor) -> Tensor:
        """A f of the batch's first n frames: [n, D, H, W], background 0 (splat_alpha_blending_forward_batch_set per chunk)"""
        fb, lib, st = self.fb, L.lib(), L.stream()
        out = torch.empty(n, self.D, self.H, self.W, dtype=torch.float32, device=fb.dev)
        final_T = fb._set_buffer(("lift", "final_T"), self.F * self.H * self.W)
        ncontrib = fb._set_buffer(("lift", "ncontrib"), self.F * self.H * self.W)       # (raw 32-bit words)
        cull = fb._set_buffer(("lift", "cull"), self.F * fb.capacity)
        for c0, cn, _ in _chunks(self.D):
            pack = fb._set_buffer(("lift", "pack"), self.F * self.N * int(lib.splat_blend_pack_floats(CHUNK)))
            L.check(lib.splat_alpha_blending_forward_batch_set(
                n, self.N, self.D, c0, cn, L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(self.opa_t),
                0, L.ptr(feature), 0, L.ptr(fb.idx_sorted), L.ptr(fb.tile_range),
                fb.capacity, 0.0, self.W, self.H, L.ptr(out), L.ptr(final_T), L.ptr(ncontrib),
                L.ptr(pack), L.ptr(cull), st))
        return out

    def _gradient_batch(self, n, feature, maps, pixel_weight, grad, loss) -> None:
        out = self._forward(n, feature)
        if pixel_weight is None:
            d = out.sub_(maps)
            r = d
        else:
            live = (pixel_weight != 0)[:, None]
            d = torch.where(live, out - maps, torch.zeros_like(out))       # selected: a pixel of weight 0 may hold NaN
            r = d * pixel_weight[:, None]
        loss.add_(0.5 * (r * d).sum())
        self._lift(n, r.contiguous(), None, grad, None)

    @torch.no_grad()
    def gradient(self, times: Sequence[float], maps: Tensor, feature: Tensor, pixel_weight: Optional[Tensor] = None,
                 _checked: bool = True, extr: Optional[Tensor] = None, intr: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """(d loss / d feature [N, D], loss [1]) of ``loss = 1/2 sum pw (A f - maps)^2`` over the frames ``times`` (``extr`` /
        ``intr``: the call's cameras, as in ``add``)"""
        times, maps, pixel_weight = self._inputs(times, maps, pixel_weight)
        cams = self._cameras(len(times), extr, intr)
        feature = self._feature(feature)
        grad = torch.zeros(self.N, self.D, dtype=torch.float32, device=self.fb.dev)
        loss = torch.zeros(1, dtype=torch.float32, device=self.fb.dev)
        for b0, n, bt, cam in self._batches(times, cams):
            self._geometry(bt, checked=_checked, cam=cam)
            self._gradient_batch(n, feature, maps[b0:b0 + n], None if pixel_weight is None else pixel_weight[b0:b0 + n], grad, loss)
        return grad, loss

    def _feature(self, feature) -> Tensor:
        if not isinstance(feature, Tensor) or tuple(feature.shape) != (self.N, self.D):
            raise ValueError(f"feature must have shape [N, D] = {(self.N, self.D)}")
        return L.need(feature.detach(), "feature")

    @torch.no_grad()
    def refine(self, times: Sequence[float], maps: Tensor, feature: Tensor, iters: int, lr: float = 0.01,
               pixel_weight: Optional[Tensor] = None, betas=(0.9, 0.999), eps: float = 1e-8, extr: Optional[Tensor] = None,
               intr: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """(feature [N, D], loss history [iters]): ``iters`` Adam steps on ``1/2 sum pw (A f - maps)^2`` from ``feature`` (the
        lifted start).  Per iteration and chunk: the forward A f (background 0), one elementwise residual, the lift kernel as
        A^T; then the project's Adam launch on [N, D].  ``history[i]`` is the loss of iteration i's feature, before its step; it
        stays on the device, and nothing synchronises with the host inside the loop (the pair capacity is settled in one pass
        over the batches before it).  Forward-only with respect to the model: refused when a model tensor requires grad.
        ``extr`` / ``intr``: the call's cameras, as in ``add``."""
        if self.model_requires_grad:
            raise ValueError("refine is forward-only with respect to the model: detach the model tensors that require grad")
        if isinstance(iters, bool) or int(iters) != iters or int(iters) < 1:
            raise ValueError("iters must be an integer >= 1")
        if not float(lr) > 0.0:
            raise ValueError("lr must be > 0")
        if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
            raise ValueError("betas must be two numbers in [0, 1)")
        if not float(eps) > 0.0:
            raise ValueError("eps must be > 0")
        times, maps, pixel_weight = self._inputs(times, maps, pixel_weight)
        f = self._feature(feature).clone()
        lib, dev = L.lib(), self.fb.dev
        batches = list(self._batches(times, self._cameras(len(times), extr, intr)))
        for _, _, bt, cam in batches:            # settles the pair capacity; a single batch keeps its lists for every iteration
            self._geometry(bt, checked=True, cam=cam)
        m, v = torch.zeros_like(f), torch.zeros_like(f)
        grad = torch.empty_like(f)
        history = torch.zeros(int(iters), dtype=torch.float32, device=dev)
        seg_end, seg_lr = (ctypes.c_int64 * 1)(f.numel()), (ctypes.c_float * 1)(float(lr))
        for it in range(int(iters)):
            grad.zero_()
            loss = history[it:it + 1]
            for b0, n, bt, cam in batches:
                if len(batches) > 1:
                    self._geometry(bt, checked=False, cam=cam)
                self._gradient_batch(n, f, maps[b0:b0 + n], None if pixel_weight is None else pixel_weight[b0:b0 + n], grad, loss)
            L.check(lib.splat_adam_step(f.numel(), L.ptr(f), L.ptr(grad), L.ptr(m), L.ptr(v), 1, seg_end,
                                        seg_lr, betas[0], betas[1], eps, it + 1, 1.0, L.stream()))
        return f, history


def lift_features(model, clock, times: Sequence[float], extr: Tensor, W: int, H: int, maps: Tensor,
                  pixel_weight: Optional[Tensor] = None, intr: Optional[Tensor] = None, **opts) -> Tuple[Tensor, Tensor]:
    """The one-call form: (feature [N, D], weight [N]) of ``FeatureLift(model, clock, extr, W, H, D, **opts)`` after one ``add``
    of the frames ``times`` with ``maps`` [F, D, H, W] and ``pixel_weight`` [F, H, W] (None: ones).  ``extr`` [4,4] / [3,4] or
    one camera per frame time [T,4,4] / [T,3,4]; ``intr`` None, [4] or [T,4]: the pinhole camera."""
    W, H = int(W), int(H)
    if W < 1 or H < 1:
        raise ValueError("W and H must be >= 1")
    times = list(times)
    _, D = _check_maps(maps, pixel_weight, len(times), None, W, H)
    per_frame = isinstance(extr, Tensor) and extr.dim() == 3 and extr.shape[0] >= 1
    if not (per_frame or intr is not None):
        return FeatureLift(model, clock, extr, W, H, D, **opts).add(times, maps, pixel_weight).result()
    from .views import _clip_cameras
    _clip_cameras(extr, intr, len(times), extr.device if isinstance(extr, Tensor) else "cpu", "T")     # before any GPU work
    lift = FeatureLift(model, clock, extr[0] if per_frame else extr, W, H, D, **opts)
    return lift.add(times, maps, pixel_weight, extr=extr, intr=intr).result()
