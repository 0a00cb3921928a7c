"""Novel-view and stereo clips: the learned video seen from elsewhere (forward only).

The reference's trainer views its dynamic model from cameras it was not trained under (src/trainer_fragGS.py):
``get_nvs_rendered_imgs`` (:1123-1155) renders frame ``i`` from camera ``i`` of a small orbit about the video camera,
``get_stereo_rendered_imgs`` (:1158-1261) renders every frame from two eyes and mixes them into an anaglyph, and
``render_video`` / ``get_interpolation_result`` are the same loop with one fixed camera (the latter at fractional times).
All of them evaluate the model and render frame by frame.

Here a clip is rendered in batches of frames with ONE camera PER FRAME of the batch (``FrameBatch.render_dynamic_sets`` with
``extr`` [F,4,4] and, for the pinhole camera, ``intr``): per batch one launch of the batched dynamic preprocess under the
frames' cameras, one binning, one sort, one compositing pass.  The two eyes of a stereo frame are two frames of the same
batch at the same time.  ``to_uint8`` / the anaglyph mix turn the float images into display-ready bytes in one launch per
batch (``splat_frames_present``): float32 arithmetic with every product and sum rounded once, restated in numpy by
tests/views_ref.py.  No CPU path, no gradients (the reference runs these under ``torch.no_grad()``).  ``pose_delta`` is the
one differentiable helper: the pose parameterisation for ``FrameBatch.render_dynamic*(camera_grad=True)``."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence

import torch
from torch import Tensor

from . import _lib as L

# Anaglyph mixes: rows = output r, g, b; columns = (left r, g, b, right r, g, b).  The five usual red-cyan matrices; the
# reference's table (:1202-1208) holds the same numbers as two 3 x 3 blocks per name and reorders them per frame (:1250).
_LUMA = (0.299, 0.587, 0.114)
_NONE = (0.0, 0.0, 0.0)
ANAGLYPH: Dict[str, tuple] = {
    "true": ((_LUMA + _NONE), (_NONE + _NONE), (_NONE + _LUMA)),
    "mono": ((_LUMA + _NONE), (_NONE + _LUMA), (_NONE + _LUMA)),
    "color": (((1.0, 0.0, 0.0) + _NONE), (_NONE + (0.0, 1.0, 0.0)), (_NONE + (0.0, 0.0, 1.0))),
    "halfcolor": ((_LUMA + _NONE), (_NONE + (0.0, 1.0, 0.0)), (_NONE + (0.0, 0.0, 1.0))),
    "optimized": (((0.0, 0.7, 0.3) + _NONE), (_NONE + (0.0, 1.0, 0.0)), (_NONE + (0.0, 0.0, 1.0))),
}
MAX_PRESENT_FRAMES = 65535          # frames of one splat_frames_present launch (the frame is grid.y)


# ---------------------------------------------------------------------------------------------------------------- cameras
def _look_at(pos: Tensor, at: Tensor) -> Tensor:
    """camera-to-world rotations [n,3,3] of cameras at ``pos`` [n,3] looking at ``at`` [3] with +y up, pytorch3d's convention:
    the COLUMNS are the camera's x, y, z (forward) axes in world coordinates; an x axis lost to an ``up`` parallel to the view
    direction is rebuilt from y x z"""
    norm = lambda v: v / v.norm(dim=1, keepdim=True).clamp_min(1e-5)
    up = torch.tensor([[0.0, 1.0, 0.0]], dtype=torch.float32).expand_as(pos)
    z = norm(at[None] - pos)
    x = norm(torch.cross(up, z, dim=1))
    y = norm(torch.cross(z, x, dim=1))
    lost = torch.isclose(x, torch.zeros_like(x), atol=5e-3).all(dim=1, keepdim=True)
    x = torch.where(lost, norm(torch.cross(y, z, dim=1)), x)
    return torch.stack((x, y, z), dim=2)


def _world_to_camera(pos: Tensor, at_z: float, device) -> Tensor:
    """extr [n,4,4] = inv([look_at(pos_i, (0, 0, at_z)) | pos_i]): the look-at in float32, the inverse in float64, the result
    float32 (the reference builds c2w in numpy float64 from the float32 rotation and inverts it there, cam_utils.py:42-62)"""
    n = pos.shape[0]
    c2w = torch.zeros(n, 4, 4, dtype=torch.float64)
    c2w[:, :3, :3] = _look_at(pos, torch.tensor([0.0, 0.0, float(at_z)], dtype=torch.float32)).double()
    c2w[:, :3, 3] = pos.double()
    c2w[:, 3, 3] = 1.0
    return torch.linalg.inv(c2w).float().contiguous().to(device)


def orbit_cameras(n: int, radius: float = 0.05, z_center: float = 1.0, turns: float = 2.0, device="cpu") -> Tensor:
    """world-to-camera matrices [n,4,4] of the reference's novel-view orbit (:1128-1134): camera i sits at
    ``radius (cos phi_i, sin phi_i, 0)`` with ``phi = linspace(0, 2 pi turns, n)`` and looks at ``(0, 0, z_center)``"""
    if int(n) < 1:
        raise ValueError("orbit_cameras: n must be positive")
    phi = torch.linspace(0, 2 * math.pi * float(turns), int(n))
    pos = torch.stack((float(radius) * torch.cos(phi), float(radius) * torch.sin(phi), torch.zeros_like(phi)), dim=1)
    return _world_to_camera(pos, z_center, device)


def stereo_cameras(radius: float = 0.05, at_z: float = 2.5, device="cpu") -> Tensor:
    """the two eyes of the reference's stereo clip (:1160-1174), [2,4,4] world to camera: phi = 0 (at +x) and pi (at -x), both
    looking at ``(0, 0, at_z)``"""
    pos = torch.tensor([[float(radius) * math.cos(p), float(radius) * math.sin(p), 0.0] for p in (0.0, math.pi)],
                       dtype=torch.float32)
    return _world_to_camera(pos, at_z, device)


def pose_delta(extr: Tensor, xi: Tensor) -> Tensor:
    """``exp(xi^) @ extr``: world-to-camera matrices ``extr`` ([F,4,4] or [4,4]) moved by the twists ``xi`` ([F,6] or [6],
    ``(omega, v)``: rotation vector, then translation), the parameterisation a pose refinement optimises.  Pure torch
    (``torch.linalg.matrix_exp`` of the 4x4 twist matrix) and differentiable w.r.t. both: the raw ``dL/dextr`` of
    ``FrameBatch.render_dynamic*(camera_grad=True)`` chains into ``xi`` by autograd.  ``xi = 0`` returns ``extr``'s bits."""
    if extr.shape[-2:] != (4, 4) or xi.shape[-1] != 6 or xi.shape[:-1] != extr.shape[:-2]:
        raise ValueError(f"pose_delta: extr [F,4,4] with xi [F,6], or [4,4] with [6]; got {tuple(extr.shape)} and {tuple(xi.shape)}")
    wx, wy, wz, vx, vy, vz = xi.unbind(-1)
    o = torch.zeros_like(wx)
    twist = torch.stack((o, -wz, wy, vx, wz, o, -wx, vy, -wy, wx, o, vz, o, o, o, o), dim=-1).reshape(*xi.shape[:-1], 4, 4)
    return torch.linalg.matrix_exp(twist).to(extr.dtype) @ extr


def canonical_intrinsics(W: int, H: int, device="cpu") -> Tensor:
    """(fx, fy, cx, cy) of the reference's canonical pinhole camera (construct_canonical_camera, cam_utils.py:42-62: fovX =
    pi / 2, fovY from the same focal length; the principal point at the image centre as camera.py builds it)"""
    fovx = math.pi / 2.0
    focal = W / (2 * math.tan(fovx / 2))
    fovy = 2 * math.atan(H / (2 * focal))
    fx, fy = W / (2 * math.tan(fovx * 0.5)), H / (2 * math.tan(fovy * 0.5))
    return torch.tensor([fx, fy, W / 2, H / 2], dtype=torch.float32, device=device)


# ---------------------------------------------------------------------------------------------------------------- bytes
def _present(a: Tensor, b: Optional[Tensor], mix: Optional[Sequence[float]], out: Optional[Tensor] = None) -> Tensor:
    a = L.need(a, "images")
    if a.dim() != 4 or a.shape[1] != 3 or a.shape[0] < 1:
        raise ValueError(f"images must be [T, 3, H, W] with T >= 1, got {tuple(a.shape)}")
    arr = None
    if b is not None:
        b = L.need(b, "right images")
        if b.shape != a.shape:
            raise ValueError(f"the two eyes differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
        arr = (ctypes.c_float * 18)(*[float(v) for v in mix])
    T, _, H, W = a.shape
    if out is None:
        out = torch.empty(T, H, W, 3, dtype=torch.uint8, device=a.device)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (T, H, W, 3) and out.is_contiguous() and out.device == a.device
    lib, st = L.lib(), L.stream()
    for t0 in range(0, T, MAX_PRESENT_FRAMES):
        n = min(MAX_PRESENT_FRAMES, T - t0)
        L.check(lib.splat_frames_present(n, H, W, L.ptr(a[t0:t0 + n]), L.ptr(None if b is None else b[t0:t0 + n]),
                                         None if arr is None else ctypes.addressof(arr), L.ptr(out[t0:t0 + n]), st))
    return out


def to_uint8(images: Tensor) -> Tensor:
    """display-ready bytes [T,H,W,3] of float images [T,3,H,W]: the float32 arithmetic of the reference's
    ``(x.clamp(0, 1) * 255).astype(np.uint8)`` (:1151-1152), a NaN giving 0"""
    return _present(images, None, None)


def _mix_matrix(mode) -> List[float]:
    if isinstance(mode, str):
        if mode not in ANAGLYPH:
            raise ValueError(f"unknown anaglyph mode {mode!r}: one of {sorted(ANAGLYPH)} or a 3 x 6 tensor")
        return [v for row in ANAGLYPH[mode] for v in row]
    m = torch.as_tensor(mode, dtype=torch.float32).detach().cpu()
    if tuple(m.shape) != (3, 6):
        raise ValueError(f"an anaglyph matrix is 3 x 6 (rows r g b over left rgb, right rgb), got {tuple(m.shape)}")
    if not bool(torch.isfinite(m).all()):
        raise ValueError("the anaglyph matrix must be finite")
    return [float(v) for v in m.reshape(-1)]


def anaglyph(left: Tensor, right: Tensor, mode="optimized") -> Tensor:
    """bytes [T,H,W,3] of the two eyes' float images [T,3,H,W] mixed by ``mode`` (a name of ``ANAGLYPH`` or a 3 x 6 tensor):
    both eyes clamped to [0, 1], ``o_c = sum_k m[c][k] (l_r l_g l_b r_r r_g r_b)[k]`` summed left to right in float32, the byte
    ``min(max(o_c * 255, 0), 255)`` truncated (the reference mixes in float64, :1250-1253; at most one level differs, on ties)"""
    return _present(left, right, _mix_matrix(mode))


# ---------------------------------------------------------------------------------------------------------------- clips
_GEO = ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")


def _video_sets(p, bg: float):
    """the reference's video row (render_iter): rgb from the SH coefficients | depth (bg 1) | mask_attribute with
    opacity.detach() when the model holds one"""
    from .layers import _colors
    sets = [dict(name="rgb", feature=_colors(p["shs"]), bg=float(bg), taps=True), dict(name="depth", feature="depth", bg=1.0)]
    m = p.get("mask_attribute")
    if isinstance(m, Tensor):
        if m.dtype != torch.float32 or m.numel() != p["position"].shape[0]:
            raise ValueError(f"mask_attribute must be float32 [N] or [N, 1], got {m.dtype} {tuple(m.shape)}")
        sets.append(dict(name="mask_attribute", feature=L.need(m.detach().reshape(-1, 1), "mask_attribute"), bg=0.0,
                         detach_opacity=True))
    return sets


def _clip_cameras(extr, intr, n: int, dev, what: str):
    """extr [4,4] / [3,4] or one per frame [n,4,4] / [n,3,4]; intr None, [4] or [n,4]; on the device, detached"""
    if not isinstance(extr, Tensor) or extr.dtype != torch.float32:
        raise ValueError("extr must be a float32 tensor")
    if extr.dim() == 3:
        if extr.shape[0] != n or tuple(extr.shape[1:]) not in ((4, 4), (3, 4)):
            raise ValueError(f"per-frame extr must be [{what} = {n}, 4, 4] or [{n}, 3, 4], got {tuple(extr.shape)}")
    elif tuple(extr.shape) not in ((4, 4), (3, 4)):
        raise ValueError(f"extr must be [4, 4], [3, 4] or one camera per frame, got {tuple(extr.shape)}")
    if intr is not None:
        if not isinstance(intr, Tensor) or intr.dtype != torch.float32 or tuple(intr.shape) not in ((4,), (n, 4)):
            raise ValueError(f"intr must be float32 (fx, fy, cx, cy), [4] or [{what} = {n}, 4]")
        intr = intr.detach().to(dev).contiguous()
    return extr.detach().to(dev).contiguous(), intr


class _Clip:
    """the model, the feature sets and the frame batch of one clip; ``batch`` renders ``F`` frames and never returns a batch
    whose tile-Gaussian pairs outgrew the pair capacity (the ``LayeredClip`` rule)"""

    def __init__(self, model, clock, W, H, sets, frames_per_batch, K, nearest, extent, bg, shs, cubic_layout, capacity, wide,
                 differentiable: bool = False):
        from .frames import FrameBatch
        from .layers import _params
        if isinstance(frames_per_batch, bool) or int(frames_per_batch) != frames_per_batch or not (1 <= int(frames_per_batch) <= 65535):
            raise ValueError("frames_per_batch must be an integer in 1 .. 65535")
        if int(W) < 1 or int(H) < 1:
            raise ValueError("W and H must be positive")
        if capacity is not None and int(capacity) < 1:
            raise ValueError("capacity must be positive")
        p, self.layout = _params(model, shs, cubic_layout, need_shs=sets is None)
        if not isinstance(model, dict) and "mask_attribute" not in p and isinstance(getattr(model, "mask_attribute", None), Tensor):
            p["mask_attribute"] = model.mask_attribute
        pos = p["position"]
        if not isinstance(pos, Tensor) or pos.dim() != 2 or pos.shape[1] != 3 or pos.shape[0] < 1:
            raise ValueError("model position must be [N, 3]")
        if not pos.is_cuda:
            raise ValueError("the model must hold CUDA (ROCm) tensors (there is no CPU path)")
        self.dev, self.clock = pos.device, clock
        self.geo = {k: p[k] for k in _GEO}
        sets = _video_sets(p, bg) if sets is None else [dict(s_) for s_ in sets]
        self.names = [s_.pop("name", None) or f"set{i}" for i, s_ in enumerate(sets)]
        if len(set(self.names)) != len(self.names) or any(n_ in ("wide", "gs_idx") for n_ in self.names):
            raise ValueError(f"set names must be distinct and none of 'wide', 'gs_idx': {self.names}")
        self.sets, self.wide = sets, wide
        self.widths = [1 if isinstance(s_["feature"], str) else int(s_["feature"].shape[-1]) for s_ in sets]
        self.F, self.W, self.H, self.K = int(frames_per_batch), int(W), int(H), int(K)
        self.nearest, self.extent = float(nearest), float(extent)
        self.fb = FrameBatch(self.F, int(pos.shape[0]), self.W, self.H, sum(self.widths), self.dev,
                             capacity=None if capacity is None else int(capacity), records=bool(differentiable))
        self.differentiable = bool(differentiable)      # False: forward only (no pair-record buffer); flow.render_flow opts in
        self.regrows = 0            # batches rendered again after their pairs outgrew the capacity

    def batch(self, times, extr: Tensor, intr: Optional[Tensor]):
        fb = self.fb
        while True:
            res = fb.render_dynamic_sets(self.clock, times, extr, self.sets, cubic_layout=self.layout, K=self.K, nearest=self.nearest,
                                         extent=self.extent, wide=self.wide, intr=intr, **self.geo,
                                         **(dict(differentiable=True) if self.differentiable else {}))
            try:
                fb.check()          # the pair counts are on the device: one synchronisation per batch
                return res
            except L.SplatError:
                # the sort dropped the surplus pairs: nothing composited from these lists is returned
                fb._grow(int(fb.pairs.max().item()))
                self.regrows += 1

    def outputs(self, T: int) -> Dict[str, Tensor]:
        f32 = dict(dtype=torch.float32, device=self.dev)
        out = {n_: torch.empty(T, w, self.H, self.W, **f32) for n_, w in zip(self.names, self.widths)}
        if self.wide is not None:
            out["wide"] = torch.empty(T, int(self.wide["feature"].shape[1]), self.H, self.W, **f32)
        if self.K > 0:
            out["gs_idx"] = torch.empty(T, self.H, self.W, self.K, dtype=torch.int32, device=self.dev)
        return out


def _padded(T: int, F: int) -> List[int]:
    return [min(i, T - 1) for i in range(((T + F - 1) // F) * F)]     # a short last batch repeats the last frame


def _batch_cameras(extr, intr, default, T: int, F: int, dev, what: str):
    """the ``_Camera`` of every batch of ``F`` frames of a call over ``T`` frame times (``layers.LayeredClip``, ``lift.FeatureLift``):
    the call's ``extr`` / ``intr``, each falling back to the object's ``default`` (extr, intr or None), checked and brought to the
    device (``_clip_cameras``), per-frame tensors padded like the frame times (``_padded``) and sliced per batch.  None: neither
    the call nor the object names a camera -- the one orthographic camera of the core entry point."""
    if extr is None and intr is None and default[1] is None:
        return None
    from .frames import _Camera
    e, i_ = _clip_cameras(default[0] if extr is None else extr, default[1] if intr is None else intr, T, dev, what)
    per_e, per_i = e.dim() == 3, i_ is not None and i_.dim() == 2
    if per_e or per_i:
        pidx = torch.tensor(_padded(T, F), device=dev)
        e = e.index_select(0, pidx) if per_e else e
        i_ = i_.index_select(0, pidx) if per_i else i_
    return [_Camera(e[b0:b0 + F] if per_e else e, i_[b0:b0 + F] if per_i else i_, F) for b0 in range(0, T, F)]


def _no_layers_with(K, wide, who: str) -> None:
    if int(K) != 0 or wide is not None:
        raise ValueError(f"{who}: neither contributor ids (K > 0) nor wide= is built for layered scenes (layers=)")


def _layered_clip(model, clock, layers, W, H, sets, frames_per_batch, nearest, extent, bg, shs, cubic_layout, capacity, extr):
    """the ``layers.LayeredClip`` of a viewed layered scene and its set names: the model and the ``sets`` default of ``_Clip``
    (``_video_sets``), the clip's batches and regrow rule; ``extr``: the call's cameras (the clip's default is the first)"""
    from .layers import LayeredClip, _params
    p, layout = _params(model, shs, cubic_layout, need_shs=sets is None)
    if not isinstance(model, dict) and "mask_attribute" not in p and isinstance(getattr(model, "mask_attribute", None), Tensor):
        p["mask_attribute"] = model.mask_attribute
    if sets is None:
        if not (isinstance(p["shs"], Tensor) and p["shs"].is_cuda):
            raise ValueError("the model must hold CUDA (ROCm) tensors (there is no CPU path)")
        sets = _video_sets(p, bg)
    sets = [dict(s_) for s_ in sets]
    names = [s_.pop("name", None) or f"set{i}" for i, s_ in enumerate(sets)]
    if len(set(names)) != len(names) or any(n_ in ("wide", "gs_idx") for n_ in names):
        raise ValueError(f"set names must be distinct and none of 'wide', 'gs_idx': {names}")
    one = extr[0] if isinstance(extr, Tensor) and extr.dim() == 3 and extr.shape[0] >= 1 else extr
    if isinstance(one, Tensor) and isinstance(p["position"], Tensor):
        one = one.to(p["position"].device)
    clip = LayeredClip(p, clock, layers, one, W, H, sets, frames_per_batch, cubic_layout=layout, nearest=nearest, extent=extent,
                       capacity=capacity)
    return clip, names


@torch.no_grad()
def render_views(model, clock, times, extr: Tensor, W: int, H: int, intr: Optional[Tensor] = None, sets=None,
                 frames_per_batch: int = 8, K: int = 0, nearest: float = 0.01, extent: float = 1.3, bg: float = 1.0,
                 shs: Optional[Tensor] = None, cubic_layout: Optional[int] = None, capacity: Optional[int] = None,
                 wide: Optional[dict] = None, stats: Optional[dict] = None, layers=None) -> Dict[str, Tensor]:
    """The clip at the frame times ``times`` (fractional times: the interpolated clip) seen from ``extr``: one world-to-camera
    matrix [4,4] for the whole clip (``render_video``) or one per time [T,4,4] (``orbit_cameras``: the novel-view clip).
    ``intr`` None: the orthographic camera of the video renderer; (fx, fy, cx, cy) as [4] or [T,4]: the pinhole camera
    (``canonical_intrinsics``).  ``model``: a parameter dict or a ``DynamicGaussians``, as ``layers.render_part`` takes it.

    ``sets``: the feature sets of ``FrameBatch.render_dynamic_sets`` (a dict may carry a ``name``); None: the reference's video
    row -- ``rgb`` from the SH coefficients (``model["shs"]`` or ``shs=``) on ``bg``, ``depth``, and ``mask_attribute`` when the
    model holds one.  ``wide``: one more detached set of any width; ``K``: contributor ids per pixel.  Returns a dict name ->
    [T,c,H,W] (``wide`` [T,c,H,W], ``gs_idx`` [T,H,W,K] when asked for), detached.

    The clip is worked through in batches of ``frames_per_batch`` frames (a short last batch is padded with its last frame, the
    padding dropped).  A batch whose tile-Gaussian pairs outgrow the pair capacity (``capacity``: the initial one; None:
    measured on the first batch) is never returned: the capacity is raised and the batch rendered again (one host
    synchronisation per batch reads the pair counts; ``stats["regrows"]`` counts them).  One orthographic camera runs the
    single-camera kernel of the training path; per-frame cameras and the pinhole camera a kernel of their own, whose conic may
    differ from the former's in the last bit.

    ``layers``: a list of ``layers.Layer`` -- the clip is the LAYERED scene (an object removed, duplicated, moved or resized)
    seen from these cameras: a ``layers.LayeredClip`` with the same ``sets`` default, batches, regrow rule and ``stats``, a set's
    feature indexed by source Gaussian.  Neither ``K > 0`` nor ``wide=`` is built for layered scenes."""
    times = [float(t) for t in times]
    T = len(times)
    if T < 1:
        raise ValueError("a clip needs at least one frame time")
    if layers is not None:
        _no_layers_with(K, wide, "render_views")
        from .layers import clip_layer_inputs
        clip_layer_inputs(layers, times)
        if isinstance(extr, Tensor):
            _clip_cameras(extr, intr, T, extr.device, "T")                   # before any GPU work
        lclip, names = _layered_clip(model, clock, layers, W, H, sets, frames_per_batch, nearest, extent, bg, shs, cubic_layout,
                                     capacity, extr)
        out = dict(zip(names, lclip.render(times, extr, intr)))
        if stats is not None:
            stats.update(regrows=lclip.regrows, capacity=lclip.fb.capacity, frame_batch_bytes=lclip.fb.memory_bytes())
        return out
    clip = _Clip(model, clock, W, H, sets, frames_per_batch, K, nearest, extent, bg, shs, cubic_layout, capacity, wide)
    extr, intr = _clip_cameras(extr, intr, T, clip.dev, "T")
    F = clip.F
    idx = torch.tensor(_padded(T, F), device=clip.dev)
    per_e, per_i = extr.dim() == 3, intr is not None and intr.dim() == 2
    if per_e:
        extr = extr.index_select(0, idx)
    if per_i:
        intr = intr.index_select(0, idx)
    out = clip.outputs(T)
    keys = clip.names + (["wide"] if wide is not None else [])
    padded = _padded(T, F)
    for b0 in range(0, T, F):
        n = min(F, T - b0)
        res = clip.batch([times[i] for i in padded[b0:b0 + F]], extr[b0:b0 + F] if per_e else extr, intr[b0:b0 + F] if per_i else intr)
        for k, r in zip(keys, res):
            out[k][b0:b0 + n].copy_(r[:n])
        if clip.K > 0:
            out["gs_idx"][b0:b0 + n].copy_(res[-1][:n])
    if stats is not None:
        stats.update(regrows=clip.regrows, capacity=clip.fb.capacity, frame_batch_bytes=clip.fb.memory_bytes())
    return out


@torch.no_grad()
def render_stereo(model, clock, times, W: int, H: int, cameras: Optional[Tensor] = None, intr: Optional[Tensor] = None,
                  mode="optimized", frames_per_batch: int = 8, nearest: float = 0.01, extent: float = 1.3, bg: float = 1.0,
                  shs: Optional[Tensor] = None, cubic_layout: Optional[int] = None, capacity: Optional[int] = None,
                  return_eyes: bool = False, layers=None):
    """The reference's stereo clip (:1158-1261): every frame time of ``times`` from the two eyes ``cameras`` ([2,4,4] world to
    camera; None: ``stereo_cameras()``), mixed into an anaglyph by ``mode`` (a name of ``ANAGLYPH`` or a 3 x 6 tensor); uint8
    [T,H,W,3].  ``intr`` None: orthographic eyes; [4]: pinhole eyes.

    A batch of ``frames_per_batch`` frames (even, >= 2) holds both eyes of ``frames_per_batch / 2`` times -- the left eyes, then
    the right eyes, so that each eye's images are one dense block --: the frame table repeats every time, one batch evaluates
    the model for both eyes, and one launch mixes the batch's images into bytes.  Only the colours are composited.
    ``return_eyes``: also return the two eyes' float images [T,3,H,W] (left, right).  Batches and the pair capacity as in
    ``render_views``.  ``layers``: a list of ``layers.Layer`` -- the stereo clip of the layered scene; each layer's times and
    per-frame deltas are repeated for the two eyes the way the clip's times are."""
    times = [float(t) for t in times]
    T = len(times)
    if T < 1:
        raise ValueError("a clip needs at least one frame time")
    if isinstance(frames_per_batch, bool) or int(frames_per_batch) != frames_per_batch or int(frames_per_batch) < 2 \
            or int(frames_per_batch) % 2:
        raise ValueError("render_stereo: frames_per_batch must be an even integer >= 2 (both eyes of a time share a batch)")
    mix = _mix_matrix(mode)
    from .layers import _params
    p, layout = _params(model, shs, cubic_layout, need_shs=True)
    if not (isinstance(p["shs"], Tensor) and p["shs"].is_cuda):
        raise ValueError("the model must hold CUDA (ROCm) tensors (there is no CPU path)")
    dev = p["shs"].device
    lt = ld = None
    if layers is not None:
        from .layers import LayeredClip, clip_layer_inputs
        _, lt, ld = clip_layer_inputs(layers, times)
        # (the clip's default camera is never used: every batch is rendered under the two eyes)
        clip = LayeredClip(p, clock, layers, torch.eye(4, device=dev), W, H, _video_sets(p, bg)[:1], frames_per_batch,
                           cubic_layout=layout, nearest=nearest, extent=extent, capacity=capacity)
    else:
        clip = _Clip(p, clock, W, H, _video_sets(p, bg)[:1], frames_per_batch, 0, nearest, extent, bg, None, layout, capacity, None)
    cams = stereo_cameras(device=dev) if cameras is None else cameras
    cams, intr = _clip_cameras(cams, intr, 2, dev, "eyes")
    if cams.dim() != 3:
        raise ValueError("cameras must hold the two eyes: [2, 4, 4] or [2, 3, 4]")
    if intr is not None and intr.dim() != 1:
        raise ValueError("render_stereo: intr is one (fx, fy, cx, cy) for both eyes")
    h = clip.F // 2
    eyes = cams.repeat_interleave(h, dim=0).contiguous()          # [L x h, R x h]
    out = torch.empty(T, H, W, 3, dtype=torch.uint8, device=dev)
    left = right = None
    if return_eyes:
        left, right = (torch.empty(T, 3, H, W, dtype=torch.float32, device=dev) for _ in range(2))
    padded = _padded(T, h)
    for b0 in range(0, T, h):
        n = min(h, T - b0)
        idx = padded[b0:b0 + h]
        bt = [times[i] for i in idx]
        if layers is not None:                                    # each layer's times and deltas: left block, then right block
            from .frames import _Camera
            rgb = clip._render_batch([tuple(t_[i] for i in idx) * 2 for t_ in lt],
                                     [None if d is None else d[idx + idx].contiguous().to(dev) for d in ld],
                                     _Camera(eyes, intr, clip.F))
        else:
            rgb = clip.batch(bt + bt, eyes, intr)[0]              # [2h,3,H,W]: the whole row of the batch, dense
        _present(rgb[:n], rgb[h:h + n], mix, out=out[b0:b0 + n])
        if return_eyes:
            left[b0:b0 + n].copy_(rgb[:n])
            right[b0:b0 + n].copy_(rgb[h:h + n])
    return (out, left, right) if return_eyes else out
