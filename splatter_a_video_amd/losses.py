"""SSIM and the L1 + D-SSIM image loss of the reference's training step, on the HIP kernels of csrc/loss.hip.

``ssim`` has the signature and the semantics of the reference's ``pointrix.model.loss.ssim`` (src/pointrix/model/loss.py:58-112):
the channel is dim -3, so the trainer's literal call ``ssim(pred.reshape(-1, h, w, 3), ...)`` (src/trainer_fragGS.py:576) slides
the window over (x, colour) planes, one per image row, and gives the trainer's number.  Inputs are read in place through their
strides (no copy).  ``dssim_l1`` is the trainer's RGB objective ``(1 - lam) * l1 + lam * (1 - ssim)`` (:575-578) in one launch.
``track_loss`` is its optical-flow term (:528-569) and ``depth_loss_dpt`` its median-normalised depth term (:589-601).
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

LAYOUTS = ("reference", "image")


def _check(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA (ROCm) tensor (there is no CPU fallback)")
    if L._cur_device is not None and t.device.index != L._cur_device():
        raise ValueError(f"{name} lives on cuda:{t.device.index} but the current device is cuda:{L._cur_device()}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
    return t


def _strides(t: torch.Tensor):
    return (ctypes.c_int64 * 4)(*t.stride())


def _scratch(N: int, Cp: int, Hp: int, Wp: int, window: int, dev) -> torch.Tensor:
    nbytes = L.lib().splat_ssim_scratch_bytes(N, Cp, Hp, Wp, window)
    if nbytes == 0:
        raise ValueError(f"ssim: unsupported sizes [{N}, {Cp}, {Hp}, {Wp}] / window {window} (odd windows 1 .. 15)")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=dev)


class _SSIM(torch.autograd.Function):
    """mean SSIM (size_average) or per-image means of [N, Cp, Hp, Wp] views; saves only the inputs, the backward is one launch
    per input that wants a gradient (SSIM is symmetric: the gradient w.r.t. img2 is the same kernel with the images swapped)"""

    @staticmethod
    def forward(ctx, img1, img2, window, size_average):
        N, Cp, Hp, Wp = img1.shape
        out = torch.empty(1 if size_average else N, dtype=torch.float32, device=img1.device)
        L.check(L.lib().splat_ssim_forward(N, Cp, Hp, Wp, window, L.ptr(img1), _strides(img1), L.ptr(img2), _strides(img2),
                                           L.ptr(out) if size_average else None, None if size_average else L.ptr(out),
                                           L.ptr(_scratch(N, Cp, Hp, Wp, window, img1.device)), L.stream()))
        ctx.save_for_backward(img1, img2)
        ctx.window, ctx.size_average = window, size_average
        return out[0] if size_average else out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        img1, img2 = ctx.saved_tensors
        N, Cp, Hp, Wp = img1.shape
        g = g.detach().to(torch.float32).contiguous()
        grads = [None, None]
        for k, (a, b) in enumerate(((img1, img2), (img2, img1))):
            if ctx.needs_input_grad[k]:
                d = torch.empty(a.shape, dtype=torch.float32, device=a.device)
                L.check(L.lib().splat_ssim_backward(N, Cp, Hp, Wp, ctx.window, L.ptr(a), _strides(a), L.ptr(b), _strides(b),
                                                    L.ptr(g), 0 if ctx.size_average else 1, L.ptr(d), _strides(d), 0,
                                                    L.stream()))
                grads[k] = d
        return grads[0], grads[1], None, None


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """SSIM of two images [N, C, H, W] (or [C, H, W] with size_average=True); C = dim -3 is the channel, the window slides over
    the last two dims.  size_average: the mean of the SSIM map (a 0-d tensor), else each image's mean ([N]).  Differentiable
    w.r.t. both images (once)."""
    _check(img1, "img1")
    _check(img2, "img2")
    if img1.shape != img2.shape:
        raise ValueError(f"ssim: shapes differ: {tuple(img1.shape)} vs {tuple(img2.shape)}")
    if img1.dim() == 3:
        if not size_average:
            raise ValueError("ssim: a [C, H, W] input has no per-image mean (size_average=False needs [N, C, H, W])")
        img1, img2 = img1.unsqueeze(0), img2.unsqueeze(0)
    if img1.dim() != 4:
        raise ValueError(f"ssim: expected [N, C, H, W] or [C, H, W], got {tuple(img1.shape)}")
    return _SSIM.apply(img1, img2, int(window_size), bool(size_average))


def planes(t: torch.Tensor, layout: str) -> torch.Tensor:
    """the [N, Cp, Hp, Wp] view of RGB frames [F, 3, H, W] whose planes the SSIM window slides over: "reference" -- the trainer's
    ``ssim(pred.permute(1, 2, 0).reshape(-1, h, w, 3))``, planes of W x 3, one per image row; "image" -- per-colour H x W"""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
    if t.dim() == 3:
        t = t.unsqueeze(0)
    return t.permute(0, 2, 3, 1) if layout == "reference" else t


def dssim_l1_grad(pred: torch.Tensor, target: torch.Tensor, w_l1: float, w_ssim: float, layout: str, grad: torch.Tensor,
                  l1_sum: torch.Tensor, ssim_sum: torch.Tensor) -> None:
    """one launch (+ the sums' reduction): grad (dense, pred's shape) = the gradient of w_l1 * mean|pred - target| +
    w_ssim * (1 - ssim(pred, target)) w.r.t. pred; sum |pred - target| and the sum of the SSIM map ADDED to the device slots"""
    _check(pred, "pred")
    _check(target, "target")
    if pred.shape != target.shape or grad.shape != pred.shape:
        raise ValueError(f"dssim_l1: pred {tuple(pred.shape)}, target {tuple(target.shape)} and grad {tuple(grad.shape)} differ")
    p4, t4, g4 = planes(pred, layout), planes(target, layout), planes(grad, layout)
    N, Cp, Hp, Wp = p4.shape
    L.check(L.lib().splat_dssim_l1_loss_grad(N, Cp, Hp, Wp, 11, L.ptr(p4), _strides(p4), L.ptr(t4), _strides(t4), w_l1,
                                             w_ssim, L.ptr(g4), _strides(g4), L.ptr(l1_sum), L.ptr(ssim_sum),
                                             L.ptr(_scratch(N, Cp, Hp, Wp, 11, pred.device)), L.stream()))


class _DSSIML1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, lam, layout):
        grad = torch.empty(pred.shape, dtype=torch.float32, device=pred.device)
        sums = torch.zeros(2, dtype=torch.float32, device=pred.device)
        dssim_l1_grad(pred, target, 1.0 - lam, lam, layout, grad, sums[0:1], sums[1:2])
        ctx.save_for_backward(grad)
        n = pred.numel()
        return (1.0 - lam) * (sums[0] / n) + lam * (1.0 - sums[1] / n)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None


def dssim_l1(pred: torch.Tensor, target: torch.Tensor, lam: float = 0.2, layout: str = "reference") -> torch.Tensor:
    """the reference trainer's RGB loss ``(1 - lam) * l1_loss(pred, target) + lam * (1 - ssim(pred, target))`` of RGB frames
    [F, 3, H, W] (or [3, H, W]; 11-tap window), its gradient w.r.t. pred computed in the same launch.  layout "reference": the
    trainer's HWC call (planes of W x 3); "image": the usual per-colour SSIM.  target is ground truth: no gradient reaches it."""
    _check(pred, "pred")
    _check(target, "target")
    if target.requires_grad:
        raise ValueError("dssim_l1: target is ground truth; detach it (no gradient w.r.t. target is computed)")
    planes(pred, layout)
    return _DSSIML1.apply(pred, target, float(lam), layout)


# ---------------------------------------------------------------------------------------------------------- the 2-D track loss
def track_loss_grad(track: torch.Tensor, targets, frame_weights: torch.Tensor, quantile: float = 0.98, scale: float = 1.0,
                    grad: torch.Tensor = None, accumulate: bool = False, per_frame: torch.Tensor = None,
                    loss_slot: torch.Tensor = None, counts: torch.Tensor = None) -> None:
    """one launch of splat_track_loss_grad (include/splat_hip.h) on the track image [F, C, H, W] (C >= 2, any strides: a channel
    slice of a wider row is read in place) and the ``tracks.TrackTargets`` of its F frame pairs.  Each output is optional:
    ``grad`` (track's shape, own strides) = scale * d(mean_f loss_f) / d track, written (accumulate=False: zeros elsewhere) or
    added at the selected pixels; ``per_frame`` [F] = loss_f; ``loss_slot`` (1 element) += mean_f loss_f; ``counts`` int32 [F, 2]
    = (visible, selected) queries per frame."""
    _check(track, "track")
    if track.dim() != 4 or track.shape[1] < 2:
        raise ValueError(f"track must be [F, C >= 2, H, W], got {tuple(track.shape)}")
    F, C, H, W = track.shape
    if (targets.F, targets.H, targets.W) != (F, H, W):
        raise ValueError(f"track targets of {targets.F} frames of {targets.W} x {targets.H} for a track image {tuple(track.shape)}")
    if targets.device != track.device:
        raise ValueError(f"track targets live on {targets.device}, the image on {track.device}")
    if not 0.0 <= float(quantile) <= 1.0:
        raise ValueError(f"quantile must be in [0, 1], got {quantile}")
    fw = frame_weights
    if not isinstance(fw, torch.Tensor) or fw.numel() != F:
        raise ValueError(f"frame_weights must be a tensor of {F} weights")
    fw = fw.to(device=track.device, dtype=torch.float32).reshape(F).contiguous()
    if grad is not None:
        _check(grad, "grad")
        if grad.shape != track.shape:
            raise ValueError(f"grad {tuple(grad.shape)} must have the track image's shape {tuple(track.shape)}")
    for t, name, n in ((per_frame, "per_frame", F), (loss_slot, "loss_slot", 1)):
        if t is not None and (_check(t, name).numel() != n or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 tensor of {n} elements")
    if counts is not None and (counts.dtype != torch.int32 or counts.numel() != 2 * F or not counts.is_contiguous()
                               or counts.device != track.device):
        raise ValueError(f"counts must be a contiguous int32 [{F}, 2] tensor on the image's device")
    lib = L.lib()
    nbytes = lib.splat_track_loss_scratch_bytes(F, targets.Q)
    if nbytes == 0:
        raise ValueError(f"track loss: unsupported sizes (F = {F}, Q = {targets.Q})")
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=track.device)
    L.check(lib.splat_track_loss_grad(F, H, W, C, L.ptr(track), _strides(track), L.ptr(targets.offsets), L.ptr(targets.pixels),
                                      L.ptr(targets.targets), targets.Q, L.ptr(fw), quantile, scale,
                                      L.ptr(grad), _strides(grad) if grad is not None else None, 1 if accumulate else 0,
                                      L.ptr(per_frame), L.ptr(loss_slot), L.ptr(counts), L.ptr(scratch), L.stream()))


def track_loss_points_grad(values: torch.Tensor, targets, frame_weights: torch.Tensor, quantile: float = 0.98, scale: float = 1.0,
                           grad: torch.Tensor = None, per_frame: torch.Tensor = None, loss_slot: torch.Tensor = None,
                           counts: torch.Tensor = None) -> None:
    """``track_loss_grad`` on PER-QUERY predictions (splat_track_loss_grad_points): ``values`` [Q, C >= 2], row i = the prediction
    of query i of ``targets`` (``tracks.TrackTargets`` of F pairs) in target order -- what
    ``FrameBatch.render_dynamic_sets(points=...)`` returns at the integer query pixels -- instead of a track image.  ``grad``
    [Q, C] = scale * d(mean_f loss_f) / d values, written in full (zeros outside the selected set and in channels >= 2); the
    other outputs as in ``track_loss_grad``.  Losses, counts and gradient rows are bit-equal to ``track_loss_grad`` on an image
    that holds the values at the query pixels; no image is filled or read."""
    _check(values, "values")
    if values.dim() != 2 or values.shape[1] < 2 or values.shape[0] != targets.Q or not values.is_contiguous():
        raise ValueError(f"values must be a contiguous [Q = {targets.Q}, C >= 2] tensor, got {tuple(values.shape)}")
    Q, C = values.shape
    F, H, W = targets.F, targets.H, targets.W
    if targets.device != values.device:
        raise ValueError(f"track targets live on {targets.device}, the values on {values.device}")
    if not 0.0 <= float(quantile) <= 1.0:
        raise ValueError(f"quantile must be in [0, 1], got {quantile}")
    fw = frame_weights
    if not isinstance(fw, torch.Tensor) or fw.numel() != F:
        raise ValueError(f"frame_weights must be a tensor of {F} weights")
    fw = fw.to(device=values.device, dtype=torch.float32).reshape(F).contiguous()
    if grad is not None:
        _check(grad, "grad")
        if grad.shape != values.shape or not grad.is_contiguous():
            raise ValueError(f"grad {tuple(grad.shape)} must be contiguous with the values' shape {tuple(values.shape)}")
    for t, name, n in ((per_frame, "per_frame", F), (loss_slot, "loss_slot", 1)):
        if t is not None and (_check(t, name).numel() != n or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 tensor of {n} elements")
    if counts is not None and (counts.dtype != torch.int32 or counts.numel() != 2 * F or not counts.is_contiguous()
                               or counts.device != values.device):
        raise ValueError(f"counts must be a contiguous int32 [{F}, 2] tensor on the values' device")
    lib = L.lib()
    nbytes = lib.splat_track_loss_scratch_bytes(F, Q)
    if nbytes == 0:
        raise ValueError(f"track loss: unsupported sizes (F = {F}, Q = {Q})")
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=values.device)
    L.check(lib.splat_track_loss_grad_points(F, H, W, C, L.ptr(values), L.ptr(targets.offsets), L.ptr(targets.pixels),
                                             L.ptr(targets.targets), Q, L.ptr(fw), quantile, scale,
                                             L.ptr(grad), L.ptr(per_frame), L.ptr(loss_slot), L.ptr(counts), L.ptr(scratch),
                                             L.stream()))


class _TrackLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, track, targets, frame_weights, quantile):
        loss = torch.zeros(1, dtype=torch.float32, device=track.device)
        grad = torch.empty(track.shape, dtype=torch.float32, device=track.device) if ctx.needs_input_grad[0] else None
        track_loss_grad(track.detach(), targets, frame_weights, quantile, 1.0, grad, loss_slot=loss)
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None


def track_loss(track_image: torch.Tensor, targets, frame_weights: torch.Tensor, quantile: float = 0.98) -> torch.Tensor:
    """the reference trainer's optical-flow term (src/trainer_fragGS.py:528-569) of F frame pairs, averaged over the pairs: per
    pair f, over the visible queries of ``targets`` (``tracks.TrackTargets``), masked_l1_loss(denormalize_coords(pred), track,
    mask=c w_f, quantile) / max(H, W) with masked_l1_loss's default normalize=True, i.e. the weighted mean
    sum_S c r / (sum_S c + 1e-8) / max(H, W), the prediction read from channels 0, 1 of ``track_image`` [F, C, H, W] (the
    rendered track_gs) at the query pixels; 0 for a pair without a visible query.  ``frame_weights`` [F]: the
    ``tracks.frame_weights`` of the pairs.  Differentiable w.r.t. the image (the quantile's selection is a constant); the
    gradient comes from the same launch."""
    _check(track_image, "track_image")
    return _TrackLoss.apply(track_image, targets, frame_weights, float(quantile))


def track_loss_sparse(uv: torch.Tensor, conic: torch.Tensor, opacity: torch.Tensor, track_gs: torch.Tensor,
                      idx_sorted: torch.Tensor, tile_range: torch.Tensor, W: int, H: int, targets, frame_weights: torch.Tensor,
                      quantile: float = 0.98, bg: float = 0.0, ordered: bool = False) -> torch.Tensor:
    """``track_loss`` of ONE frame pair without the dense track image: ``track_gs`` [P, C >= 2] (its first three channels at
    most) is composited at the integer query pixels of ``targets`` only (``gs.alpha_blending_points(differentiable=True)``),
    the [Q, C'] result is scattered into a zero [1, C', H, W] image and handed to ``track_loss`` -- which reads nothing but
    those pixels, so value and gradients are the dense route's ``track_loss(alpha_blending(...)[None, :3], ...)``.
    ``opacity`` is detached, as the reference does for its attribute blend.  Differentiable w.r.t. ``uv``, ``conic`` and
    ``track_gs``; the backward adds with float atomics (it raises in deterministic mode) unless ``ordered=True``, which is
    passed on to ``gs.alpha_blending_points`` (no float atomic, a fixed order of every sum; needs the sort's pair map)."""
    from .gs.raster_ops import alpha_blending_points
    if targets.F != 1:
        raise ValueError(f"track_loss_sparse takes the targets of one frame pair, got {targets.F}")
    W, H = int(W), int(H)
    if (targets.H, targets.W) != (H, W):
        raise ValueError(f"track targets of a {targets.W} x {targets.H} image for W, H = {W}, {H}")
    _check(track_gs, "track_gs")
    if track_gs.dim() != 2 or track_gs.shape[1] < 2:
        raise ValueError(f"track_gs must be [P, C >= 2], got {tuple(track_gs.shape)}")
    if targets.device != track_gs.device:
        raise ValueError(f"track targets live on {targets.device}, track_gs on {track_gs.device}")
    feat = track_gs[:, :3]
    C = feat.shape[1]
    pix = targets.pixels.long()
    points = torch.stack([pix % W, pix // W], dim=1).to(torch.float32)       # integer pixels: one corner of weight 1
    vals = alpha_blending_points(uv, conic, opacity.detach(), feat, idx_sorted, tile_range, bg, W, H, points, differentiable=True,
                                 ordered=ordered)
    image = torch.zeros(C, H * W, dtype=torch.float32, device=track_gs.device).index_copy(1, pix, vals.t())
    return track_loss(image.view(1, C, H, W), targets, frame_weights, quantile)


# ------------------------------------------------------------------------------------- the median-normalised depth loss
DEPTH_CHUNK = 4096          # pixels one workgroup of the depth kernels handles (DPT_CH of csrc/loss.hip)


def _depth_frames(t: torch.Tensor, name: str) -> torch.Tensor:
    """the [F, 1, H, W] view the depth kernels read: an [F, 1, H, W] tensor as it is; any other shape is ONE frame of numel
    pixels (the reference's semantics: the trainer passes [H, W, 1]), viewed as [1, 1, rows, cols] in place where its strides
    allow a 2-D view (else copied)"""
    _check(t, name)
    if t.dim() == 4 and t.shape[1] == 1:
        return t
    s = t.squeeze()
    if s.dim() > 2:
        try:
            s = s.view(-1, s.shape[-1])
        except RuntimeError:
            s = s.reshape(-1, s.shape[-1])
    while s.dim() < 2:
        s = s.unsqueeze(0)
    return s[None, None]


def _depth_scratch(F: int, H: int, W: int, dev) -> torch.Tensor:
    nbytes = L.lib().splat_depth_dpt_scratch_bytes(F, H, W)
    if nbytes == 0:
        raise ValueError(f"depth loss: unsupported sizes (F = {F}, H = {H}, W = {W}; H W <= 2^31 - 1, F <= 2^24)")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=dev)


def _depth_out(t, name: str, n: int, dev, dtype=torch.float32) -> None:
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of {n} elements on the image's device")


def depth_stats(img: torch.Tensor) -> torch.Tensor:
    """[F, 2] = (lower median, mean absolute deviation from it) of every frame of ``img`` [F, 1, H, W] (any strides; any other
    shape: one frame) -- splat_depth_stats.  For ground-truth depth, which is fixed per video frame: compute once, hand it to
    ``depth_dpt_loss_grad`` / the training step as ``gt_stats``."""
    v = _depth_frames(img.detach(), "img")
    F, _, H, W = v.shape
    out = torch.empty(F, 2, dtype=torch.float32, device=v.device)
    L.check(L.lib().splat_depth_stats(F, H, W, L.ptr(v), _strides(v), L.ptr(out), L.ptr(_depth_scratch(F, H, W, v.device)),
                                      L.stream()))
    return out


def depth_dpt_loss_grad(pred: torch.Tensor, gt: torch.Tensor, scale: float = 1.0, grad: torch.Tensor = None,
                        accumulate: bool = False, per_frame: torch.Tensor = None, loss_slot: torch.Tensor = None,
                        gt_stats: torch.Tensor = None, stats: torch.Tensor = None, ties: torch.Tensor = None) -> None:
    """splat_depth_dpt_loss_grad (include/splat_hip.h) on depth frames ``pred``, ``gt`` [F, 1, H, W] (any strides, read in
    place).  Each output is optional: ``grad`` (pred's shape, own strides) = scale * d(mean_f loss_f) / d pred, written in full
    or (accumulate) added; ``per_frame`` [F] = loss_f; ``loss_slot`` (1 element) += mean_f loss_f; ``stats`` [F, 4] = t_p, s_p,
    t_g, s_g; ``ties`` int32 [F] = the number of pixels equal to the median.  ``gt_stats`` [F, 2]: ``depth_stats(gt)``, cached."""
    _check(pred, "pred")
    _check(gt, "gt")
    if pred.dim() != 4 or pred.shape[1] != 1 or gt.shape != pred.shape:
        raise ValueError(f"pred and gt must both be [F, 1, H, W], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    F, _, H, W = pred.shape
    dev = pred.device
    if grad is not None:
        _check(grad, "grad")
        if grad.shape != pred.shape:
            raise ValueError(f"grad {tuple(grad.shape)} must have pred's shape {tuple(pred.shape)}")
    _depth_out(per_frame, "per_frame", F, dev)
    _depth_out(loss_slot, "loss_slot", 1, dev)
    _depth_out(gt_stats, "gt_stats", 2 * F, dev)
    _depth_out(stats, "stats", 4 * F, dev)
    _depth_out(ties, "ties", F, dev, torch.int32)
    L.check(L.lib().splat_depth_dpt_loss_grad(F, H, W, L.ptr(pred), _strides(pred), L.ptr(gt), _strides(gt), L.ptr(gt_stats),
                                              scale, L.ptr(grad), _strides(grad) if grad is not None else None,
                                              1 if accumulate else 0, L.ptr(per_frame), L.ptr(loss_slot), L.ptr(stats),
                                              L.ptr(ties), L.ptr(_depth_scratch(F, H, W, dev)), L.stream()))


class _DepthDPT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        loss = torch.zeros(1, dtype=torch.float32, device=pred.device)
        grad = torch.empty(pred.shape, dtype=torch.float32, device=pred.device) if ctx.needs_input_grad[0] else None
        depth_dpt_loss_grad(pred.detach(), gt, 1.0, grad, loss_slot=loss)
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


def depth_loss_dpt(pred_depth: torch.Tensor, gt_depth: torch.Tensor, weight=None) -> torch.Tensor:
    """the reference's ``depth_loss_dpt(pred_depth, gt_depth)`` (src/loss.py:184-207; the trainer's depth term,
    src/trainer_fragGS.py:600): the mean squared difference of the two images after each is shifted by its median and scaled by
    its mean absolute deviation from it.  A tensor of any shape is one frame of numel pixels (the trainer passes [H, W, 1]);
    [F, 1, H, W] gives the mean of the F frames' losses.  Strided views are read in place.  Differentiable w.r.t. pred_depth
    (once), the paths through the median and the scale included; the gradient comes from the same launches.  gt_depth is ground
    truth: no gradient reaches it.  ``weight`` (which the trainer never passes) is not implemented."""
    if weight is not None:
        raise NotImplementedError("depth_loss_dpt: the optional weight map is not implemented (the trainer never passes it)")
    _check(pred_depth, "pred_depth")
    _check(gt_depth, "gt_depth")
    if gt_depth.requires_grad:
        raise ValueError("depth_loss_dpt: gt_depth is ground truth; detach it (no gradient w.r.t. gt_depth is computed)")
    if pred_depth.shape != gt_depth.shape:
        raise ValueError(f"depth_loss_dpt: shapes differ: {tuple(pred_depth.shape)} vs {tuple(gt_depth.shape)}")
    return _DepthDPT.apply(_depth_frames(pred_depth, "pred_depth"), _depth_frames(gt_depth, "gt_depth"))


class _FlowL1(torch.autograd.Function):
    """mean over the maps of the weighted-mean L1; the forward's one call also writes the gradient (scale = 1 / T)"""

    @staticmethod
    def forward(ctx, pred, gt, weight):
        from .flow import flow_error_sums
        sums, grad = flow_error_sums(pred.detach(), gt, weight, scale=1.0 / pred.shape[0], want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        return (sums[:, 0] / sums[:, 2].clamp_min(1e-30)).mean().to(torch.float32)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def flow_l1(pred: torch.Tensor, gt: torch.Tensor, weight=None) -> torch.Tensor:
    """the trainer's earlier flow term ``masked_l1_loss(pred_flow, gt_flow, weights)`` (src/trainer_fragGS.py:525-526) on flow
    maps [T, 2, H, W]: per map ``sum w (|du| + |dv|) / sum w`` (``weight`` [T, H, W]; None: 1), then the mean over the maps; a
    map whose weights are all zero contributes 0.  One call each way (csrc/flow.hip: float32 partials of 2048 pixels folded in
    float64 in a fixed order, no float atomics: bit-reproducible).  Differentiable w.r.t. ``pred`` (once); ``gt`` and
    ``weight`` are data."""
    _check(pred, "pred")
    _check(gt, "gt")
    if gt.requires_grad or (isinstance(weight, torch.Tensor) and weight.requires_grad):
        raise ValueError("flow_l1: gt and weight are data; detach them (no gradient with respect to them is computed)")
    return _FlowL1.apply(pred, gt, weight)
