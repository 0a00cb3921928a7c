"""Appearance editing: fit the SH colours of frozen geometry to an edited frame, then render the clip with them.

The reference does this in ``optimize_appearance_from_mask`` / ``optimize_appearance_from_img`` (src/trainer_fragGS.py:999-1120):
up to 1000 iterations of render frame 0, ``F.mse_loss`` against the edited image, backward, Adam at lr 0.0025 on the SH
coefficients alone, until the loss drops below 1e-4 -- the whole renderer and its whole backward per iteration, for tensors that
are frozen.  Here the frame's geometry is binned and sorted ONCE, and an iteration is

    compute_sh forward (selected rows) -> splat_blend_fit_color (composite + MSE residual + per-pair colour gradient, one launch,
    only the tiles whose list holds a selected Gaussian) -> splat_tile_loss_sum -> splat_pair_records_segment_sum ->
    compute_sh backward (selected rows) -> splat_adam_step (selected rows)

with no host synchronisation; the loss history stays on the device and is read every ``check_every`` iterations.  No float
atomics anywhere: two fits of the same inputs give the same bits, with ``splat_set_deterministic(1)`` or without.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple, Union

import torch
from torch import Tensor

from . import _lib as L

SH_COEFFS = 16          # degree 3, as the renderer evaluates it (dptr_ortho_enhanced.py:272)
_CTOR_OPTIONS = ("bg", "lr", "betas", "eps", "sh_rows", "pixel_weight", "active_only")
_RUN_OPTIONS = ("max_iters", "tol", "check_every")


def _num_tiles(W: int, H: int) -> int:
    return ((W + 15) // 16) * ((H + 15) // 16)


def select_gaussians(gs_idx: Tensor, mask: Tensor, P: int) -> Tensor:
    """bool [P]: true for every Gaussian id that ``gs_idx`` ([H, W, K], or [1, H, W, K] as ``render_batch`` returns it) lists
    at a pixel with ``mask > 0``; the padding id -1 is dropped.  The reference's ``torch.unique(gs_idx[0][mask > 0])`` without
    the sort (src/trainer_fragGS.py:1014-1015).  Plain torch, CPU or GPU tensors."""
    if not isinstance(gs_idx, Tensor) or not isinstance(mask, Tensor):
        raise TypeError("gs_idx and mask must be tensors")
    if gs_idx.dim() == 4:
        if gs_idx.shape[0] != 1:
            raise ValueError("gs_idx with a batch dimension must be [1, H, W, K]")
        gs_idx = gs_idx[0]
    if gs_idx.dim() != 3 or gs_idx.dtype not in (torch.int32, torch.int64):
        raise ValueError("gs_idx must be an integer tensor [H, W, K] or [1, H, W, K]")
    if tuple(mask.shape) != tuple(gs_idx.shape[:2]):
        raise ValueError(f"mask must have shape [H, W] = {tuple(gs_idx.shape[:2])}, got {tuple(mask.shape)}")
    P = int(P)
    if P < 0:
        raise ValueError("P must be >= 0")
    ids = gs_idx[mask > 0].reshape(-1).long()
    ids = ids[ids >= 0]
    if ids.numel() and int(ids.max()) >= P:
        raise ValueError(f"gs_idx names Gaussian {int(ids.max())}, P = {P}")
    sel = torch.zeros(P, dtype=torch.bool, device=gs_idx.device)
    sel[ids] = True
    return sel


def _check_run_options(max_iters, tol, check_every) -> Tuple[int, float, int]:
    if int(max_iters) != max_iters or int(max_iters) < 1:
        raise ValueError("max_iters must be an integer >= 1")
    tol = float(tol)
    if not tol == tol or tol == float("inf"):
        raise ValueError("tol must be a finite number (or -inf: never stop early)")
    if int(check_every) != check_every or int(check_every) < 1:
        raise ValueError("check_every must be an integer >= 1")
    return int(max_iters), tol, int(check_every)


def _check_fit_options(lr, betas, eps, sh_rows) -> None:
    if sh_rows not in ("all", "dc"):
        raise ValueError('sh_rows must be "all" or "dc"')
    if not float(lr) > 0.0:
        raise ValueError("lr must be > 0")
    if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError("betas must be two numbers in [0, 1)")
    if not float(eps) > 0.0:
        raise ValueError("eps must be > 0")


def blend_fit_color(uv: Tensor, conic: Tensor, opacity: Tensor, feature: Tensor, idx_sorted: Tensor, tile_range: Tensor,
                    slot_sorted: Tensor, bg: float, W: int, H: int, target: Tensor, tile_loss: Tensor, pair_grad: Tensor,
                    pixel_weight: Optional[Tensor] = None, active_tiles: Optional[Tensor] = None, n_active: Optional[int] = None,
                    out: Optional[Tensor] = None, ncontrib: Optional[Tensor] = None) -> None:
    """splat_blend_fit_color on the current stream (include/splat_hip.h): composites ``feature`` [P, 3], writes every launched
    tile's share of the MSE against ``target`` [H, W, 3] to ``tile_loss`` [T] and of dL/dcolour to ``pair_grad`` [M, 4] at the
    pair slots; ``active_tiles`` int32 [n] names the tiles to launch (None: all of them).  ``n_active`` defaults to the length of
    ``active_tiles``; an empty list launches nothing."""
    uv, conic, opacity, feature = L.need(uv, "uv"), L.need(conic, "conic"), L.need(opacity, "opacity"), L.need(feature, "feature")
    idx_sorted, tile_range = L.need(idx_sorted, "idx_sorted", torch.int32), L.need(tile_range, "tile_range", torch.int32)
    slot_sorted = L.need(slot_sorted, "slot_sorted", torch.int32)
    target = L.need(target, "target")
    W, H = int(W), int(H)
    if W < 1 or H < 1:
        raise ValueError("W and H must be >= 1")
    if feature.dim() != 2:
        raise ValueError("feature must have shape [P, 3]")
    P, C = feature.shape
    T, M = _num_tiles(W, H), idx_sorted.numel()
    if uv.numel() != 2 * P or conic.numel() != 3 * P or opacity.numel() != P:
        raise ValueError("uv [P,2] / conic [P,3] / opacity [P] / feature [P,3] must agree on P")
    if tile_range.numel() != 2 * T:
        raise ValueError("tile_range must have shape [ceil(W/16)*ceil(H/16), 2]")
    if slot_sorted.numel() != M:
        raise ValueError("slot_sorted must have one entry per idx_sorted entry")
    if tuple(target.shape) != (H, W, 3):
        raise ValueError(f"target must have shape [H, W, 3] = {(H, W, 3)}, got {tuple(target.shape)}")
    for name, t, numel, dt in (("tile_loss", tile_loss, T, torch.float32), ("pair_grad", pair_grad, 4 * M, torch.float32),
                               ("pixel_weight", pixel_weight, H * W, torch.float32), ("out", out, 3 * H * W, torch.float32),
                               ("ncontrib", ncontrib, H * W, torch.int32), ("active_tiles", active_tiles, None, torch.int32)):
        if t is None:
            continue
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or (numel is not None and t.numel() != numel):
            raise ValueError(f"{name} must be a contiguous {dt} GPU tensor of {numel if numel is not None else 'n_active'} elements")
    if active_tiles is None:
        n, at = (T if n_active is None else int(n_active)), None
    else:
        n = active_tiles.numel() if n_active is None else int(n_active)
        if n > active_tiles.numel():
            raise ValueError("n_active exceeds the length of active_tiles")
        at = active_tiles
        if n == 0:
            return      # (an empty tensor has no address to tell it from "every tile")
    L.check(L.lib().splat_blend_fit_color(
        P, C, L.ptr(uv), L.ptr(conic), L.ptr(opacity), L.ptr(feature), L.ptr(idx_sorted), L.ptr(tile_range),
        L.ptr(slot_sorted), M, bg, W, H, L.ptr(target), L.ptr(pixel_weight), n, L.ptr(at),
        L.ptr(tile_loss), L.ptr(pair_grad), L.ptr(out), L.ptr(ncontrib), L.stream()))


class AppearanceFit:
    """The colours of one frame's frozen geometry fitted to an edited image of that frame.

    ``uv, depth, conic, radius, tiles, opacity``: the frame's geometry as ``gs.preprocess_ortho`` / ``frame_preprocess`` return
    it (``tiles`` is accepted for parity with ``sort_gaussian`` and not read).  ``shs`` [P, 16, 3]; ``selected`` bool [P], the
    Gaussians whose colours are trained (None: all).  ``sh_rows="all"`` trains all 16 coefficient rows
    (optimize_appearance_from_mask), ``"dc"`` only row 0 (optimize_appearance_from_img: ``features_rest.requires_grad = False``).
    ``lr, betas, eps``: Adam as ``torch.optim.Adam`` defines it (the reference: lr 0.0025, defaults otherwise).
    ``pixel_weight`` [H, W] weighs the pixels' squared errors (None: ones, ``F.mse_loss``).  ``active_only``: only the tiles
    whose list holds a selected Gaussian run in an iteration; the other tiles' share of the loss is a constant, computed once
    per ``run``.

    The constructor bins and sorts once (with the pair map), evaluates all colours once and flags the active tiles.
    ``run(target)`` starts with one launch over ALL tiles (the loss of the inactive ones depends on the target) and goes on
    over the active ones.  Colours are evaluated for the renderer's constant view direction (0, 0, 1)."""

    def __init__(self, uv: Tensor, depth: Tensor, conic: Tensor, radius: Tensor, tiles: Optional[Tensor], opacity: Tensor,
                 shs: Tensor, selected: Optional[Tensor], W: int, H: int, bg: float = 0.0, lr: float = 0.0025,
                 betas=(0.9, 0.999), eps: float = 1e-8, sh_rows: str = "all", pixel_weight: Optional[Tensor] = None,
                 active_only: bool = True):
        _check_fit_options(lr, betas, eps, sh_rows)
        W, H = int(W), int(H)
        if W < 1 or H < 1:
            raise ValueError("W and H must be >= 1")
        for name, t in (("uv", uv), ("depth", depth), ("conic", conic), ("radius", radius), ("opacity", opacity), ("shs", shs)):
            if not isinstance(t, Tensor):
                raise TypeError(f"{name} must be a torch.Tensor")
        if shs.dim() != 3 or tuple(shs.shape[1:]) != (SH_COEFFS, 3):
            raise ValueError(f"shs must have shape [P, {SH_COEFFS}, 3], got {tuple(shs.shape)}")
        P = shs.shape[0]
        if P < 1:
            raise ValueError("shs holds no Gaussian")
        if uv.numel() != 2 * P or depth.numel() != P or conic.numel() != 3 * P or radius.numel() != P or opacity.numel() != P:
            raise ValueError(f"uv [P,2] / depth [P] / conic [P,3] / radius [P] / opacity [P] must agree with shs on P = {P}")
        if selected is not None and (not isinstance(selected, Tensor) or selected.dtype != torch.bool or tuple(selected.shape) != (P,)):
            raise ValueError(f"selected must be a bool tensor [P = {P}] or None")
        if pixel_weight is not None and (not isinstance(pixel_weight, Tensor) or tuple(pixel_weight.shape) != (H, W)):
            raise ValueError(f"pixel_weight must have shape [H, W] = {(H, W)}")
        from .gs.raster_ops import sort_gaussian_capped
        from .renderer import OrthoEnhancedRenderer
        self.W, self.H, self.P, self.T = W, H, P, _num_tiles(W, H)
        self.bg, self.lr, self.betas, self.eps = float(bg), float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.dc = sh_rows == "dc"
        self.uv, self.conic = L.need(uv.detach(), "uv"), L.need(conic.detach(), "conic")
        self.opacity = L.need(opacity.detach(), "opacity")
        self.shs = L.need(shs.detach(), "shs")
        self.pixel_weight = None if pixel_weight is None else L.need(pixel_weight.detach(), "pixel_weight")
        dev = self.uv.device
        # bin and sort once; only the pairs whose tile the splat can reach with alpha >= 1/255 (reach masks)
        self.idx_sorted, self.tile_range, status = sort_gaussian_capped(self.uv, L.need(depth.detach(), "depth"), W, H,
                                                                        L.need(radius.detach(), "radius", torch.int32), None,
                                                                        self.conic, self.opacity)
        self.M = self.idx_sorted.numel()
        if self.M == 0 or status.pairmap is None:
            raise ValueError("no Gaussian reaches the frame: nothing to fit")
        self.goff, self.slot_sorted = status.pairmap.goff, status.pairmap.slot_sorted
        sel = torch.ones(P, dtype=torch.bool, device=dev) if selected is None else selected.to(dev)
        self.sel_idx = torch.nonzero(sel).reshape(-1)              # int64; one host sync, set-up
        self.S = S = self.sel_idx.numel()
        if S == 0:
            raise ValueError("the selection is empty: nothing to fit")
        self.all_selected = S == P
        self.feature = OrthoEnhancedRenderer.colors(self.shs)       # [P, 3], every colour once
        self.shs_sel = self.shs.index_select(0, self.sel_idx).contiguous()
        self.dirs = torch.zeros(S, 3, dtype=torch.float32, device=dev)
        self.dirs[:, 2] = 1.0
        self.vis = torch.ones(S, dtype=torch.uint8, device=dev)
        self.clamped = torch.empty(S, 3, dtype=torch.uint8, device=dev)
        self.colors_sel = self.feature if self.all_selected else torch.empty(S, 3, dtype=torch.float32, device=dev)
        self.dcolor = torch.empty(P, 4, dtype=torch.float32, device=dev)
        self.dcol_sel = torch.empty(S, 4, dtype=torch.float32, device=dev)
        self.g_col = torch.empty(S, 3, dtype=torch.float32, device=dev)
        self.dshs = torch.empty(S, SH_COEFFS, 3, dtype=torch.float32, device=dev)
        self.pair_grad = torch.zeros(self.M, 4, dtype=torch.float32, device=dev)
        self.tile_loss = torch.zeros(self.T, dtype=torch.float32, device=dev)
        if self.dc:     # the trainable block, compact: coefficient row 0 of the selected Gaussians
            self.param = self.shs_sel[:, 0, :].contiguous()
            self.g_param = torch.empty_like(self.param)
        else:
            self.param, self.g_param = self.shs_sel, self.dshs
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.param), torch.zeros_like(self.param)
        self.seg_end = (ctypes.c_int64 * 1)(self.param.numel())
        self.seg_lr = (ctypes.c_float * 1)(self.lr)
        self.step = 0
        # a tile is active when its list holds a selected Gaussian
        if active_only and not self.all_selected:
            hit = torch.zeros(self.M + 1, dtype=torch.int64, device=dev)
            hit[1:] = torch.cumsum(sel[self.idx_sorted.long()].to(torch.int64), 0)
            tr = self.tile_range.long().clamp(0, self.M)
            self.active_tiles = torch.nonzero(hit[tr[:, 1]] > hit[tr[:, 0]]).reshape(-1).to(torch.int32).contiguous()
            self.n_active = self.active_tiles.numel()
        else:
            self.active_tiles, self.n_active = None, self.T

    def _iteration(self, target: Tensor, history: Tensor, slot: int, all_tiles: bool) -> None:
        lib, st = L.lib(), L.stream()
        S = self.S
        L.check(lib.splat_compute_sh_forward(S, L.ptr(self.shs_sel), 3, L.ptr(self.dirs), L.ptr(self.vis), 0,
                                             L.ptr(self.colors_sel), L.ptr(self.clamped), st))
        if not self.all_selected:
            self.feature.index_copy_(0, self.sel_idx, self.colors_sel)
        at = None if all_tiles else self.active_tiles
        blend_fit_color(self.uv, self.conic, self.opacity, self.feature, self.idx_sorted, self.tile_range, self.slot_sorted, self.bg,
                        self.W, self.H, target, self.tile_loss, self.pair_grad, self.pixel_weight, at)
        L.check(lib.splat_tile_loss_sum(self.T, L.ptr(self.tile_loss), L.ptr(history), slot, st))
        L.check(lib.splat_pair_records_segment_sum(self.P, 4, L.ptr(self.pair_grad), L.ptr(self.goff), L.ptr(self.dcolor), st))
        torch.index_select(self.dcolor, 0, self.sel_idx, out=self.dcol_sel)
        self.g_col.copy_(self.dcol_sel[:, :3])
        L.check(lib.splat_compute_sh_backward(S, L.ptr(self.shs_sel), 3, L.ptr(self.dirs), L.ptr(self.vis),
                                              L.ptr(self.clamped), 0, L.ptr(self.g_col), 0, L.ptr(self.dshs), L.ptr(None), st))
        if self.dc:
            self.g_param.copy_(self.dshs[:, 0, :])
        self.step += 1
        L.check(lib.splat_adam_step(self.param.numel(), L.ptr(self.param), L.ptr(self.g_param), L.ptr(self.exp_avg),
                                    L.ptr(self.exp_avg_sq), 1, self.seg_end, self.seg_lr, self.betas[0],
                                    self.betas[1], self.eps, self.step, 1.0, st))
        if self.dc:
            self.shs_sel[:, 0, :].copy_(self.param)

    @torch.no_grad()
    def run(self, target: Tensor, max_iters: int = 1000, tol: float = 1e-4, check_every: int = 10) -> Tuple[Tensor, Tensor, int]:
        """(shs_fitted [P, 16, 3], losses [iterations], iterations).  ``losses[i]`` is the loss of iteration i's colours, before
        its Adam step, as the reference prints it.  The history is read every ``check_every`` iterations (and after the last),
        and the fit stops when a value since the last check is below ``tol``: up to ``check_every - 1`` iterations more than
        the reference, which synchronises on ``loss.item()`` every iteration; ``check_every=1`` stops exactly where it does.
        Rows of ``shs`` that are not selected (and with ``sh_rows="dc"`` rows 1 .. 15) keep their bits.  A second ``run``
        continues from the fitted colours and the optimizer state of the first."""
        max_iters, tol, check_every = _check_run_options(max_iters, tol, check_every)
        target = L.need(target.detach(), "target")
        if tuple(target.shape) != (self.H, self.W, 3):
            raise ValueError(f"target must have shape [H, W, 3] = {(self.H, self.W, 3)}, got {tuple(target.shape)}")
        history = torch.zeros(max_iters, dtype=torch.float32, device=target.device)
        done, checked = 0, 0
        for it in range(max_iters):
            self._iteration(target, history, it, all_tiles=(it == 0))
            done = it + 1
            if done % check_every == 0 or done == max_iters:
                below = bool((history[checked:done] < tol).any().item())     # the only host synchronisation
                checked = done
                if below:
                    break
        fitted = self.shs.clone()
        fitted.index_copy_(0, self.sel_idx, self.shs_sel)
        return fitted, history[:done].clone(), done


def _model_params(model, shs: Optional[Tensor], cubic_layout: Optional[int]):
    from .dynamics import GAUSSIAN_MAJOR, SEGMENT_MAJOR, DynamicGaussians
    from .tracking import _NAMES
    if isinstance(model, DynamicGaussians):
        p = {k: getattr(model, k).detach() for k in _NAMES}
        layout = model.cubic_layout if cubic_layout is None else int(cubic_layout)
        extra = getattr(model, "shs", None)
    elif isinstance(model, dict):
        missing = [k for k in _NAMES if k not in model]
        if missing:
            raise ValueError(f"model lacks {missing}")
        p = {k: (v.detach() if isinstance(v, Tensor) else v) for k, v in model.items()}
        layout = GAUSSIAN_MAJOR if cubic_layout is None else int(cubic_layout)
        extra = model.get("shs")
    else:
        raise TypeError("model must be a parameter dict or DynamicGaussians")
    if layout not in (GAUSSIAN_MAJOR, SEGMENT_MAJOR):
        raise ValueError("cubic_layout must be GAUSSIAN_MAJOR or SEGMENT_MAJOR")
    shs = extra if shs is None else shs
    if not isinstance(shs, Tensor):
        raise ValueError("no SH coefficients: the model holds no 'shs'; pass shs=")
    p["shs"] = shs.detach()
    return p, layout


def fit_appearance(model, clock, time, extr: Tensor, W: int, H: int, target: Tensor, mask: Optional[Tensor] = None,
                   num_idx: int = 10, shs: Optional[Tensor] = None, cubic_layout: Optional[int] = None, nearest: float = 0.01,
                   extent: float = 1.3, **fit_options) -> Tuple[Dict[str, Tensor], Tensor]:
    """Fit the colours of a dynamic model to ``target`` [H, W, 3], an edited image of frame ``time``.

    ``model``: a parameter dict (position, pos_cubic_node, rotation, rot_poly_feat, rot_fourier_feat, opacity (logit), scaling
    (log), shs [N, 16, 3]) or a ``DynamicGaussians`` (which holds no SH: pass ``shs=``), as ``tracking.track_pixels`` takes it.
    With ``mask`` [H, W] this is optimize_appearance_from_mask: frame ``time`` is rendered once with ``num_idx`` ids per pixel,
    the Gaussians listed under ``mask > 0`` are selected and all their SH rows fitted.  Without it, optimize_appearance_from_img:
    all Gaussians, the DC row only.  ``fit_options``: ``AppearanceFit``'s bg, lr, betas, eps, sh_rows, pixel_weight, active_only
    and ``run``'s max_iters, tol, check_every.

    Returns (the parameter dict with ``shs`` replaced -- every other entry the input's own tensor --, the loss history); render
    the clip from it with the renderers or ``FrameBatch``."""
    unknown = [k for k in fit_options if k not in _CTOR_OPTIONS + _RUN_OPTIONS]
    if unknown:
        raise ValueError(f"unknown fit options {unknown}; known: {_CTOR_OPTIONS + _RUN_OPTIONS}")
    ctor = {k: v for k, v in fit_options.items() if k in _CTOR_OPTIONS}
    run = {k: v for k, v in fit_options.items() if k in _RUN_OPTIONS}
    ctor.setdefault("sh_rows", "all" if mask is not None else "dc")
    _check_fit_options(ctor.get("lr", 0.0025), ctor.get("betas", (0.9, 0.999)), ctor.get("eps", 1e-8), ctor["sh_rows"])
    _check_run_options(run.get("max_iters", 1000), run.get("tol", 1e-4), run.get("check_every", 10))
    W, H, num_idx = int(W), int(H), int(num_idx)
    if W < 1 or H < 1:
        raise ValueError("W and H must be >= 1")
    if num_idx < 1:
        raise ValueError("num_idx must be >= 1")
    if not isinstance(target, Tensor) or tuple(target.shape) != (H, W, 3):
        raise ValueError(f"target must have shape [H, W, 3] = {(H, W, 3)}")
    if mask is not None and (not isinstance(mask, Tensor) or tuple(mask.shape) != (H, W)):
        raise ValueError(f"mask must have shape [H, W] = {(H, W)}")
    p, layout = _model_params(model, shs, cubic_layout)
    N = p["position"].shape[0]
    if p["shs"].dim() != 3 or tuple(p["shs"].shape) != (N, SH_COEFFS, 3):
        raise ValueError(f"shs must have shape [N = {N}, {SH_COEFFS}, 3]")
    from .dynamics import frame_preprocess
    from .tracking import _cull_args
    near_p, ext_p = _cull_args(nearest, extent)
    with torch.no_grad():
        uv, depth, conic, radius, tiles, opa = frame_preprocess(
            clock, time, L.need(extr, "extr"), W, H, position=L.need(p["position"], "position"),
            pos_cubic_node=L.need(p["pos_cubic_node"], "pos_cubic_node"), rotation=p["rotation"], rot_poly_feat=p["rot_poly_feat"],
            rot_fourier_feat=p["rot_fourier_feat"], opacity=p["opacity"], scaling=p["scaling"], nearest=near_p, extent=ext_p,
            cubic_layout=layout)
        selected = None
        if mask is not None:
            from .gs.raster_ops import alpha_blending_enhanced, sort_gaussian_capped
            from .renderer import OrthoEnhancedRenderer
            idx_sorted, tile_range, _ = sort_gaussian_capped(uv, depth, W, H, radius, None, conic, opa)
            _, _, gs_idx = alpha_blending_enhanced(uv, conic, opa, OrthoEnhancedRenderer.colors(L.need(p["shs"], "shs")), idx_sorted,
                                                   tile_range, float(ctor.get("bg", 0.0)), W, H, K=num_idx)
            selected = select_gaussians(gs_idx, mask.to(gs_idx.device), N)
        fit = AppearanceFit(uv, depth, conic, radius, tiles, opa, p["shs"], selected, W, H, **ctor)
        fitted, losses, _ = fit.run(target, **run)
    out = dict(p)
    out["shs"] = fitted
    return out, losses
