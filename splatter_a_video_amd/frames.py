"""Frame-batched rendering: F frames of one Gaussian set through ONE set of kernel launches (SURVEY 7 stage 6).

The reference renders the frames of a batch one after the other (``render_batch``,
src/pointrix/renderer/dptr_ortho_enhanced.py:385-433: ~13 native launches and ~80 eager kernels per frame).  Here every
kernel of the per-frame path -- orthographic preprocess, tile binning, per-tile sort, record packing, compositing
forward, compositing backward -- takes the frame as a grid dimension, and the Gaussian-side backward (pair reduce +
preprocess backward) runs once per batch: a batch costs the launches of one frame, the short kernels fill the chip, and
the compositing kernels see F x T tiles in one launch (no half-empty last round of workgroups).  Same images and
gradients as F calls of the per-frame operators (tests/test_gpu_frames.py).

``FrameBatch`` owns the batch's device buffers (allocated once, ~140 MB per 480p frame of 300k Gaussians); ``render`` is
autograd-aware and crosses the C ABI ONCE per direction (``splat_frames_forward`` / ``splat_frames_backward``: the struct
``splat_frames_t`` carries every pointer); ``render_sets`` / ``render_dynamic`` compose the ``*_batch`` entry points.
No CPU fallback.
"""
from __future__ import annotations

import ctypes
import inspect
import os
import warnings
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib as L
from .gs.fused_ops import check_sink
from .gs.point_ops import _extr12, _points


# splat_frames_t carries every pointer of a batch for the one-call entry points (the library checks ``struct_bytes``
# against its own sizeof); both structs are built from the header's text
_SplatFrames = L.HEADER.structs["splat_frames_t"]
_SplatCamera = L.HEADER.structs["splat_camera_t"]


def _versions(*tensors):
    """(tensor, autograd version) of the camera / offset tensors a backward re-reads WITHOUT save_for_backward (they are
    passed as raw pointers): an in-place edit between forward and backward would silently change the gradients"""
    return tuple((t, t._version) for t in tensors if t is not None)


def _check_versions(saved, what: str) -> None:
    for t, v in saved:
        if t._version != v:
            raise RuntimeError(f"FrameBatch: {what} was modified in place between the forward and its backward (the backward "
                               "re-projects under the forward's cameras / offsets); clone it before editing")


class _Camera:
    """Camera of a batch: ``extr`` one world-to-camera matrix ([4,4] / [3,4]) or one per frame ([F,4,4] / [F,3,4] -- the
    reference's render_batch gives every batch element its own, dptr_ortho_enhanced.py:409-411); ``intr`` None: the
    orthographic camera of the video renderer, else the pinhole camera's (fx, fy, cx, cy), [4] or [F,4]."""

    def __init__(self, extr: Tensor, intr: Optional[Tensor], F: int):
        extr = L.need(extr, "extr")
        if extr.dim() == 3:
            if extr.shape[0] != F or tuple(extr.shape[1:]) not in ((4, 4), (3, 4)):
                raise ValueError(f"per-frame extr must be [F={F}, 4, 4] or [F, 3, 4]")
            self.extr_fs = int(extr.shape[1] * extr.shape[2])
        else:
            if extr.numel() < 12:
                raise ValueError("extr must hold at least 3x4 floats (row-major [R|T])")
            self.extr_fs = 0
        self.extr = extr
        self.intr, self.intr_fs = None, 0
        if intr is not None:
            intr = L.need(intr, "intr")
            if intr.dim() == 2:
                if tuple(intr.shape) != (F, 4):
                    raise ValueError(f"per-frame intr must be [F={F}, 4]")
                self.intr_fs = 4
            elif intr.numel() < 4:
                raise ValueError("intr must be [fx, fy, cx, cy]")
            self.intr = intr
        self.perspective = intr is not None

    def struct(self, offsets: Optional[Tensor] = None) -> _SplatCamera:
        c = _SplatCamera()
        c.perspective = 1 if self.perspective else 0
        c.intr = None if self.intr is None else self.intr.data_ptr()
        c.intr_frame_stride = self.intr_fs
        c.extr = self.extr.data_ptr()
        c.extr_frame_stride = self.extr_fs
        c.offsets = None if offsets is None else offsets.data_ptr()
        return c

    def tensors(self):
        return (self.extr,) if self.intr is None else (self.extr, self.intr)


def _constant_camera(extr, intr, F: int, who: str) -> Optional[_Camera]:
    """the camera of a differentiable dynamic batch: None for the one orthographic camera ([4,4] / [3,4] without intr: the path
    that was always differentiable), else a ``_Camera``.  Cameras are constants -- one that requires grad raises instead of
    being detached silently (camera-pose gradients are not built)."""
    if any(isinstance(t, Tensor) and t.requires_grad for t in (extr, intr)):
        raise ValueError(f"{who}: the cameras are constants (no gradient with respect to extr / intr is built); pass them "
                         "detached")
    if intr is None and not (isinstance(extr, Tensor) and extr.dim() == 3):
        return None
    return _Camera(extr, intr, F)


class _CameraGrad:
    """``camera_grad=True`` of a differentiable dynamic batch: the cameras as the kernel of include/splat_hip_camera_grad.h reads
    them (always a ``_Camera``, also for the one orthographic camera, whose parameter gradients stay with the core entry
    point), the shapes the gradients go back in, and the ``grad_sink`` buffers of ``extr`` / ``intr``."""

    def __init__(self, extr, intr, sink: Dict[str, Tensor], F: int, who: str):
        if not isinstance(extr, Tensor) or tuple(extr.shape) not in ((4, 4), (3, 4), (F, 4, 4), (F, 3, 4)):
            raise ValueError(f"{who}: camera_grad=True takes extr [4,4] / [3,4] / [F,4,4] / [F,3,4] (F = {F})")
        if intr is not None and (not isinstance(intr, Tensor) or tuple(intr.shape) not in ((4,), (F, 4))):
            raise ValueError(f"{who}: camera_grad=True takes intr [4] / [F,4] (F = {F})")
        self.cam = _Camera(extr.detach(), None if intr is None else intr.detach(), F)
        self.versions = _versions(*self.cam.tensors())
        self.extr_shape, self.intr_shape = tuple(extr.shape), (None if intr is None else tuple(intr.shape))
        self.sink_extr, self.sink_intr = sink.get("extr"), sink.get("intr")
        for name, buf, shape in (("extr", self.sink_extr, self.extr_shape), ("intr", self.sink_intr, self.intr_shape)):
            if buf is None:
                continue
            if shape is None or tuple(buf.shape) != shape or buf.dtype != torch.float32 or not buf.is_cuda or not buf.is_contiguous():
                raise ValueError(f"{who}: grad_sink[{name!r}] must be a contiguous float32 GPU buffer of {name}'s shape")

    def one_ortho(self) -> bool:
        """the one orthographic camera: the parameters' backward is the core entry point (its bits)"""
        return not self.cam.perspective and self.cam.extr_fs == 0

    def backward(self, fb: "FrameBatch", rec: Tensor, stride: int, depth_column: int, tab, position, cubic, layout: int, I: int,
                 rotation, rot_poly, rot_fourier, scaling, need_extr: bool, need_intr: bool):
        """(dL/dextr, dL/dintr) in the tensors' shapes from the batch's pair records -- after the tile, sparse and wide backward
        have filled them.  A sink receives its gradient by ADDITION and None goes back to autograd; a camera nobody asks about
        launches nothing."""
        want_e = need_extr or self.sink_extr is not None
        want_i = self.cam.perspective and (need_intr or self.sink_intr is not None)
        if not (want_e or want_i):
            return None, None
        _check_versions(self.versions, "a camera tensor")
        lib, F = L.lib(), fb.F
        de = torch.zeros(F if self.cam.extr_fs else 1, 12, dtype=torch.float32, device=fb.dev) if want_e else None
        di = torch.zeros(F if self.cam.intr_fs else 1, 4, dtype=torch.float32, device=fb.dev) if want_i else None
        part = fb._set_buffer(("camera_grad", "partials"), int(lib.splat_camera_grad_partials_floats(F, fb.P)))
        L.check(lib.splat_frames_camera_backward_dynamic(
            F, fb.P, I, fb.W, fb.H, fb.capacity, stride, depth_column, L.ptr(rec), L.ptr(fb.goff), L.ptr(tab), L.ptr(position),
            L.ptr(cubic), layout, L.ptr(rotation), L.ptr(rot_poly), L.ptr(rot_fourier), L.ptr(scaling),
            ctypes.byref(self.cam.struct()), L.ptr(part), L.ptr(de), L.ptr(di), L.stream()))
        g_e = g_i = None
        if want_e:
            if self.extr_shape[-2] == 4:                     # the bottom row of a 4x4 gets zeros
                g_e = torch.zeros(self.extr_shape, dtype=torch.float32, device=fb.dev)
                g_e[..., :3, :] = de.reshape(self.extr_shape[:-2] + (3, 4))
            else:
                g_e = de.reshape(self.extr_shape)
            if self.sink_extr is not None:
                self.sink_extr.add_(g_e)
                g_e = None
        if want_i:
            g_i = di.reshape(self.intr_shape)
            if self.sink_intr is not None:
                self.sink_intr.add_(g_i)
                g_i = None
        return (g_e if need_extr else None), (g_i if need_intr else None)


def _camera_grad(extr, intr, grad_sink, F: int, who: str):
    """(``_CameraGrad``, the forward's camera -- None: the one orthographic camera --, grad_sink without the camera names)"""
    sink = dict(grad_sink or {})
    cams = {k: sink.pop(k) for k in ("extr", "intr") if k in sink}
    cg = _CameraGrad(extr, intr, cams, F, who)
    return cg, (None if cg.one_ortho() else cg.cam), (sink or None)


# python-level switch of the multi-set paths (tests flip it in code -- no environment variable is read; the library's own
# options: L.set_option)
# "reach": create only the (Gaussian, tile) pairs whose tile the splat can reach with alpha >= 1/255 (splat_bin_*_batch_reach:
# a third fewer pairs on the bench scene, same images / ids / gradients); False: the reference's bounding-square pairs
OPTIONS = {"sets_one_pass": True, "reach": True}


def _set_tensors(sets, points, wide) -> list:
    """every feature tensor a render call was handed (sets, the sparse and the wide set), before any parsing: what autograd could
    attach a backward to"""
    out = []
    for s_ in list(sets or []) + [points, wide]:
        f = s_.get("feature") if isinstance(s_, dict) else None
        out += list(f) if isinstance(f, (list, tuple)) else [f]
    return [t for t in out if isinstance(t, Tensor)]


def _tiles(W: int, H: int) -> int:
    return ((W + 15) // 16) * ((H + 15) // 16)


class FrameBatch:
    """Buffers and launch sequence of a batch of ``F`` frames of ``P`` Gaussians at ``W`` x ``H`` with ``C`` composited
    feature channels (C <= 32).  ``capacity`` = tile-Gaussian pairs reserved per frame; None: measured on the first call
    (one host sync), afterwards the batch runs without any host synchronisation and ``check()`` (call it whenever the
    host synchronises anyway, e.g. once per optimiser step) raises if a frame outgrew it; without ``check()`` the next
    forward raises, a step or a few late (the flag travels to pinned host memory behind the binning kernels; the error is
    raised once and the flag cleared, so batches that fit keep running afterwards).  An overflow of the LAST batches of a run
    is only seen by ``check()``: call it after the final step.

    ``records=False``: a FORWARD-ONLY batch.  The backward's pair-record buffer ([F, capacity, stride] floats, half of a
    batch's memory at video sizes) is never allocated -- no forward launch reads or writes it -- and every differentiable render
    (``differentiable=True`` / ``camera_grad=True``, or grad mode with an input that requires grad) raises ``ValueError`` before
    a launch.  The forward-only clip renderers (``layers.LayeredClip``, ``lift.FeatureLift``, ``views``) build theirs this way."""

    def __init__(self, F: int, P: int, W: int, H: int, C: int, device, capacity: Optional[int] = None,
                 want_abs: bool = False, slack: float = 1.25, records: bool = True):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("FrameBatch lives on the GPU (there is no CPU path)")
        if not (1 <= C <= 32):
            raise ValueError("1 <= C <= 32 feature channels per batch")
        self.F, self.P, self.W, self.H, self.C = int(F), int(P), int(W), int(H), int(C)
        self.T = _tiles(W, H)
        self.dev, self.want_abs, self.slack = dev, bool(want_abs), float(slack)
        self.records = bool(records)
        lib = L.lib()
        f32, i32 = torch.float32, torch.int32
        F_, P_, T_ = self.F, self.P, self.T
        self.uv = torch.empty(F_, P_, 2, dtype=f32, device=dev)
        self.depth = torch.empty(F_, P_, 1, dtype=f32, device=dev)
        self.conic = torch.empty(F_, P_, 3, dtype=f32, device=dev)
        self.radius = torch.empty(F_, P_, dtype=i32, device=dev)
        self.tile_range = torch.empty(F_, T_, 2, dtype=i32, device=dev)
        self.pairs = torch.zeros(F_, dtype=i32, device=dev)          # M of every frame (device)
        self.overflow = torch.zeros(1, dtype=i32, device=dev)
        self.bin_bytes = int(lib.splat_bin_scratch_bytes(P_, W, H))
        self.bin_scratch = torch.empty(F_ * self.bin_bytes, dtype=torch.uint8, device=dev)
        self.goff = torch.empty(F_, P_, dtype=i32, device=dev)
        self.reach = torch.empty(F_, P_, dtype=i32, device=dev)      # reach words of the count step for the sort step
        self.pack = torch.empty(F_ * P_ * int(lib.splat_blend_pack_floats(C)), dtype=f32, device=dev)
        self.out = None
        self.final_T = torch.empty(F_, H, W, dtype=f32, device=dev)
        self.ncontrib = torch.empty(F_, H, W, dtype=i32, device=dev)
        self.ncp = int(lib.splat_blend_pair_stride(C, 1 if want_abs else 0, 0))
        self.tap = torch.zeros(P_, 2, dtype=f32, device=dev)         # densification taps of the last backward
        self.abs_tap = torch.zeros(P_, 2, dtype=f32, device=dev) if want_abs else None
        self.radii_max = torch.zeros(P_, dtype=i32, device=dev)
        self.capacity = None
        self.keys = self.owner = self.idx_sorted = self.slot_sorted = self.pair_records = self.cull_flags = None
        # one forward, one backward: every render* call overwrites the batch's buffers (sorted lists, packed records, final_T,
        # ncontrib, cull flags ...) that its own backward reads.  `generation` counts the forwards; a backward whose forward
        # is not the latest one raises instead of silently using another call's lists.
        self.generation = 0
        if capacity is not None:
            self._reserve(int(capacity))

    # ------------------------------------------------------------------ buffers that depend on the pair capacity
    def _reserve(self, capacity: int) -> None:
        dev, F_ = self.dev, self.F
        self.capacity = int(capacity)
        self.keys = torch.empty(F_, capacity, dtype=torch.int64, device=dev)
        self.owner = torch.empty(F_, capacity, dtype=torch.int32, device=dev)
        self.idx_sorted = torch.empty(F_, capacity, dtype=torch.int32, device=dev)
        self.slot_sorted = torch.empty(F_, capacity, dtype=torch.int32, device=dev)
        # read and written by the backward alone (the tile backward fills it, the Gaussian-side backward folds it)
        self.pair_records = torch.empty(F_ * capacity * self.ncp, dtype=torch.float32, device=dev) if self.records else None
        self.cull_flags = torch.empty(F_, capacity, dtype=torch.int32, device=dev)   # the forward's cull, for the backward

    def _grow(self, pairs: int) -> None:
        """size the pair buffers for a fullest frame of ``pairs`` tile-Gaussian pairs: the one place of the capacity rule"""
        self._reserve(int(pairs * self.slack) + 1024)

    def _bin_and_sort_fitting(self, opacity: Tensor, checked: bool = True) -> int:
        """``_bin_and_sort`` until the lists fit (the forward-only clips: the sort drops surplus pairs, and nothing may be
        composited or folded in from truncated lists): ``check()`` reads the pair counts -- one host synchronisation per batch --
        and a batch that outgrew the capacity is binned again with a larger one.  Returns the number of regrows.  ``checked``
        False: one pass, nothing is read."""
        regrows = 0
        while True:
            self._bin_and_sort(opacity)
            if not checked:
                return regrows
            try:
                self.check()
                return regrows
            except L.SplatError:
                self._grow(int(self.pairs.max().item()))
                regrows += 1

    def _set_buffer(self, key, numel: int) -> Tensor:
        """scratch of the multi-set backward (pair records / packed records per feature set), kept across steps"""
        cache = self.__dict__.setdefault("_set_buffers", {})
        t = cache.get(key)
        if t is None or t.numel() < numel:
            t = torch.empty(numel, dtype=torch.float32, device=self.dev)
            cache[key] = t
        return t

    def check(self) -> int:
        """host sync; raises when a frame's pairs exceeded the capacity (its surplus pairs were dropped), else returns the
        largest per-frame pair count"""
        m = int(self.pairs.max().item())
        if self.capacity is not None and m > self.capacity:
            self.overflow.zero_()                   # reported here: the sticky flag must not fail the next batch again
            self._ovf_event = None
            raise L.SplatError(f"FrameBatch: {m} tile-Gaussian pairs in one frame exceed the capacity {self.capacity}")
        return m

    def _begin_forward(self) -> int:
        self._poll_overflow()
        self.generation += 1
        return self.generation

    def _note_overflow(self) -> None:
        """behind the binning kernels of a forward: the overflow flag travels to pinned host memory asynchronously.  The
        device flag is sticky (bin_scatter only ever sets it), so ONE copy in flight is enough: while an earlier copy has not
        completed no new one is enqueued -- a host that runs ahead of the GPU still polls an event that WILL complete (replacing
        the pending event on every forward left it polling events that never had)."""
        if torch.cuda.is_current_stream_capturing():
            return                                  # (inside a HIP-graph capture nothing may be polled: call check() after a replay)
        ev = getattr(self, "_ovf_event", None)
        if ev is not None and not ev.query():
            return                                  # the copy in flight is older than this batch; the next one sees its flag
        if ev is not None:
            self._read_overflow()                   # a completed copy nobody polled yet
        if getattr(self, "_ovf_host", None) is None:
            self._ovf_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._ovf_host.copy_(self.overflow, non_blocking=True)
        self._ovf_event = torch.cuda.Event()
        self._ovf_event.record()

    def _read_overflow(self) -> None:
        """the completed host copy of the flag: raise once, then clear the device flag so that later batches that fit run
        again (a caller may catch the error, e.g. to rebuild with more slack)"""
        self._ovf_event = None
        if int(self._ovf_host[0]) != 0:
            self._ovf_host[0] = 0
            self.overflow.zero_()                   # stream-ordered behind the kernels that set it
            raise L.SplatError(f"FrameBatch: a batch held more tile-Gaussian pairs in one frame than the capacity "
                               f"{self.capacity} (its surplus pairs were dropped: images and gradients of that batch -- an earlier "
                               "one, possibly also the one just enqueued: the flag is sticky -- were incomplete); build the batch "
                               "with a larger `capacity` / `slack`")

    def _poll_overflow(self) -> None:
        """at the next forward, without a host synchronisation: raises if an earlier batch outgrew the capacity -- a caller
        that never calls check() still learns of it a few steps late instead of never"""
        if torch.cuda.is_current_stream_capturing():
            return
        ev = getattr(self, "_ovf_event", None)
        if ev is not None and ev.query():
            self._read_overflow()

    def _check_generation(self, gen: int) -> None:
        if gen != self.generation:
            raise L.SplatError(
                f"FrameBatch: backward of render call #{gen} after render call #{self.generation} on the same batch -- the later "
                "forward has overwritten the buffers this backward reads (sorted lists, packed records, final_T, ncontrib).  "
                "A FrameBatch holds ONE forward at a time: run the backward before the next render* (also under no_grad), or "
                "use one FrameBatch per micro-batch.")

    def memory_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in vars(self).values() if isinstance(t, Tensor))

    def _forward_only_guard(self, who: str, tensors, asked: bool = False) -> None:
        """a batch without the pair-record buffer (``records=False``) has no backward: refuse, before any launch, a render that
        asks for one (``asked``) or that autograd would attach one to"""
        if getattr(self, "records", True):
            return
        if asked or (torch.is_grad_enabled() and any(isinstance(t, Tensor) and t.requires_grad for t in tensors)):
            raise ValueError(f"{who}: this FrameBatch was built with records=False (forward only: it holds no pair-record buffer "
                             "for a backward); render under torch.no_grad() with detached tensors, or build the batch with "
                             "records=True")

    # ------------------------------------------------------------------ forward / backward launch sequences
    def _geometry(self, xyz, scales, uquats, offsets, cam: "_Camera", nearest, extent, opacity=None, op_fs=0, measure=False):
        """fused preprocess (projection + cov3d + EWA under the batch's camera) + tile binning + per-tile depth sort of all frames"""
        lib, st = L.lib(), L.stream()
        F_, P_, W, H = self.F, self.P, self.W, self.H
        L.check(lib.splat_preprocess_forward_batch_cam(
            F_, P_, L.ptr(xyz), L.ptr(offsets), L.ptr(scales), L.ptr(uquats), ctypes.byref(cam.struct()), W,
            H, nearest, extent, L.ptr(self.uv), L.ptr(self.depth), L.ptr(self.conic), L.ptr(self.radius), st))
        self._bin_and_sort(opacity, op_fs, measure)

    def _bin_and_sort(self, opacity: Optional[Tensor] = None, op_fs: int = 0, measure: bool = False):
        """tile binning + per-tile depth sort of all frames.  With ``opacity`` ([P], or per frame [F,P] with ``op_fs`` = P) and
        OPTIONS["reach"]: only the pairs whose tile the splat can reach with alpha >= 1/255 are created.  ``measure``: read
        the pair counts between the two steps (one host sync, as ``gs.sort_gaussian`` makes) and grow the pair buffers when a
        frame holds more pairs than they were sized for -- no pair is dropped, no overflow is flagged."""
        lib, st = L.lib(), L.stream()
        F_, P_, W, H = self.F, self.P, self.W, self.H
        reach = opacity is not None and OPTIONS["reach"]
        if reach:
            L.check(lib.splat_bin_count_batch_reach(
                F_, P_, L.ptr(self.uv), L.ptr(self.radius), L.ptr(self.conic), L.ptr(opacity), op_fs,
                W, H, L.ptr(self.bin_scratch), L.ptr(self.tile_range), L.ptr(self.pairs), L.ptr(None),
                L.ptr(self.reach), st))
        else:
            L.check(lib.splat_bin_count_batch(F_, P_, L.ptr(self.uv), L.ptr(self.radius), W, H,
                                              L.ptr(self.bin_scratch), L.ptr(self.tile_range), L.ptr(self.pairs), st))
        if measure:
            m = int((self.pairs if F_ == 1 else self.pairs.max()).item())
            if self.capacity is None or m > self.capacity:
                self._grow(m)
        elif self.capacity is None:    # first batch: size the pair buffers (the only host sync of the object's life)
            self._grow(int(self.pairs.max().item()))
        cap = self.capacity
        if reach:
            L.check(lib.splat_bin_sort_batch_reach(
                F_, P_, L.ptr(self.uv), L.ptr(self.depth), L.ptr(self.radius), L.ptr(self.reach), W, H,
                L.ptr(self.bin_scratch), L.ptr(self.tile_range),
                cap, L.ptr(self.keys), L.ptr(self.idx_sorted), L.ptr(self.overflow), L.ptr(self.goff),
                L.ptr(self.owner), L.ptr(self.slot_sorted), st))
        else:
            L.check(lib.splat_bin_sort_batch(
                F_, P_, L.ptr(self.uv), L.ptr(self.depth), L.ptr(self.radius), W, H,
                L.ptr(self.bin_scratch), L.ptr(self.tile_range), cap, L.ptr(self.keys), L.ptr(self.idx_sorted),
                L.ptr(self.overflow), L.ptr(self.goff), L.ptr(self.owner), L.ptr(self.slot_sorted), st))
        if not measure:                # (a measured batch fits: there is no flag to bring home)
            self._note_overflow()

    def _struct(self, xyz, scales, uquats, opacity, feature, offsets, cam, bg, nearest=0.01, extent=1.3) -> _SplatFrames:
        b = _SplatFrames()
        extr = cam.extr
        b.extr_frame_stride, b.intr_frame_stride = cam.extr_fs, cam.intr_fs
        b.intr = None if cam.intr is None else cam.intr.data_ptr()
        b.perspective = 1 if cam.perspective else 0
        b.struct_bytes = ctypes.sizeof(_SplatFrames)
        b.F, b.P, b.W, b.H, b.C = self.F, self.P, self.W, self.H, self.C
        b.want_abs = 1 if self.want_abs else 0
        b.capacity = self.capacity or 0
        b.nearest, b.extent, b.bg = nearest, extent, bg
        b.stream = L.stream()
        dp = lambda t: None if t is None else t.data_ptr()
        for name, t in dict(xyz=xyz, offsets=offsets, scales=scales, uquats=uquats, opacity=opacity, feature=feature, extr=extr,
                            uv=self.uv, depth=self.depth, conic=self.conic, radius=self.radius, bin_scratch=self.bin_scratch,
                            tile_range=self.tile_range, pairs=self.pairs, overflow=self.overflow, goff_incl=self.goff,
                            owner=self.owner, idx_sorted=self.idx_sorted, slot_sorted=self.slot_sorted, keys=self.keys,
                            pack=self.pack, final_T=self.final_T, ncontrib=self.ncontrib, pair_records=self.pair_records,
                            tap=self.tap, abs_tap=self.abs_tap, radii_max=self.radii_max,
                            cull_flags=self.cull_flags,
                            reach=self.reach if (opacity is not None and OPTIONS["reach"]) else None).items():
            setattr(b, name, dp(t))
        return b

    def _forward_onecall(self, xyz, scales, uquats, opacity, feature, offsets, cam, bg, nearest, extent):
        """the whole forward of the batch behind ONE crossing of the C ABI (splat_frames_forward).  A batch of
        ``frame_rasterization``'s pool (``_measured``) runs the same launches step by step instead, with the pair counts read
        in between (``_bin_and_sort(measure=True)``) -- except inside a stream capture, where nothing may synchronise."""
        lib = L.lib()
        if getattr(self, "_measured", False) and not torch.cuda.is_current_stream_capturing():
            self._geometry(xyz, scales, uquats, offsets, cam, nearest, extent, opacity, 0, measure=True)
            out = torch.empty(self.F, self.C, self.H, self.W, dtype=torch.float32, device=self.dev)
            L.check(lib.splat_alpha_blending_forward_batch(
                self.F, self.P, self.C, L.ptr(self.uv), L.ptr(self.conic), L.ptr(opacity), 0, L.ptr(feature), 0,
                L.ptr(self.idx_sorted), L.ptr(self.tile_range), self.capacity, bg, L.ptr(None), self.W, self.H, 0, 0, L.ptr(out),
                L.ptr(self.final_T), L.ptr(self.ncontrib), L.ptr(None), L.ptr(self.pack), L.ptr(self.cull_flags), L.stream()))
            return out
        if self.capacity is None:      # first batch: size the pair buffers (the only host sync of the object's life)
            L.check(lib.splat_frames_count(ctypes.byref(self._struct(xyz, scales, uquats, opacity, feature, offsets, cam, bg,
                                                                     nearest, extent))))
            self._grow(int(self.pairs.max().item()))
        out = torch.empty(self.F, self.C, self.H, self.W, dtype=torch.float32, device=self.dev)
        b = self._struct(xyz, scales, uquats, opacity, feature, offsets, cam, bg, nearest, extent)
        b.out = out.data_ptr()
        L.check(lib.splat_frames_forward(ctypes.byref(b)))
        self._note_overflow()
        return out

    def _backward_onecall(self, dL_dout, xyz, scales, uquats, offsets, cam, bg, bufs, accumulate, dbg=None):
        b = self._struct(xyz, scales, uquats, None, None, offsets, cam, bg)
        b.accumulate = 1 if accumulate else 0
        b.dL_dout = dL_dout.data_ptr()
        b.d_xyz, b.d_scales, b.d_uquats = bufs["xyz"].data_ptr(), bufs["scales"].data_ptr(), bufs["uquats"].data_ptr()
        b.d_opacity, b.d_feature = bufs["opacity"].data_ptr(), bufs["feature"].data_ptr()
        b.dbg_T_front = None if dbg is None else dbg.data_ptr()
        L.check(L.lib().splat_frames_backward(ctypes.byref(b)))

    # ------------------------------------------------------------------ public
    def render(self, xyz: Tensor, scales: Tensor, uquats: Tensor, opacity: Tensor, feature: Tensor, offsets: Optional[Tensor],
               extr: Tensor, bg: float = 0.0, nearest: float = 0.01, extent: float = 1.3,
               grad_sink: Optional[Dict[str, Tensor]] = None, intr: Optional[Tensor] = None) -> Tensor:
        """images [F,C,H,W] of the F frames ``xyz + offsets[f]`` (static scale / rotation / opacity / feature [P,C]) under
        the orthographic camera ``extr`` -- or, with ``intr`` (fx, fy, cx, cy), the pinhole camera of gs.rasterization.
        ``extr`` / ``intr`` may hold one camera per frame ([F,4,4] / [F,4]: render_batch's per-element cameras,
        dptr_ortho_enhanced.py:409-411); ``offsets`` may then be None.  With one orthographic camera the Gaussian-side
        backward runs its projection chain once per batch, otherwise once per frame (cameras are not differentiated).  Differentiable w.r.t. xyz, scales, uquats, opacity, feature; the backward ADDS
        the gradients of the names found in ``grad_sink`` into those buffers instead (e.g. FlatGradBucket views; autograd
        then sees no gradient for them), the others are returned to autograd.  After
        the backward, ``tap`` / ``abs_tap`` hold the batch's summed densification taps and ``radii_max`` the largest
        screen radius of every Gaussian over the frames."""
        self._forward_only_guard("render", (xyz, scales, uquats, opacity, feature, offsets), bool(grad_sink))
        sink = check_sink(grad_sink, {"xyz": xyz, "scales": scales, "uquats": uquats, "opacity": opacity, "feature": feature})
        return _RenderFrames.apply(xyz, scales, uquats, opacity, feature, offsets, extr, self, float(bg), float(nearest),
                                   float(extent), sink, intr)


    def fuse_l1(self, targets, weights, sums: Tensor) -> None:
        """arm the LOSS-FUSED backward for the next backward pass of a ``render_sets`` / ``render_dynamic_sets`` forward: the
        image gradients of ``sum_s weights[s] * mean |out[s] - targets[s]|`` (the reference's l1_loss terms, src/trainer_fragGS.py:
        573-600) are derived inside the tile kernel from the forward's output row and the target images ``targets[s]``
        [F, c_s, H, W]; ``sums`` [F, tiles, 3] receives sum |out - target| per frame, tile and routing group (tap set, second
        set, detached set; every entry is written: add them up).  Call ``torch.autograd.backward(outputs, fb.l1_placeholders())`` afterwards: the gradient tensors handed to
        the backward are placeholders (no gradient image is written or read)."""
        self._l1 = dict(targets=list(targets), weights=list(weights), sums=sums)

    def l1_placeholders(self, widths=None):
        """zero-stride gradient tensors of the sets' shapes for a loss-fused backward (no memory behind them)"""
        ws = widths or [3, 1, self.C - 4]
        z = torch.zeros(1, dtype=torch.float32, device=self.dev)
        return [z.expand(self.F, w, self.H, self.W) for w in ws]

    # ------------------------------------------------------------------ dynamic Gaussians (rows a15 + f1)
    def frame_table(self, clock, times) -> Tensor:
        """device table of the per-frame scalars (segment, offset inside it, time bases) of ``times`` (cached)"""
        key = (id(clock), tuple(float(t) for t in times))
        cache = self.__dict__.setdefault("_tables", {})
        tab = cache.get(key)
        if tab is None:
            import numpy as np
            if len(times) != self.F:
                raise ValueError(f"the batch holds {self.F} frames")
            host = np.zeros((self.F, 16), np.float32)
            for f, t in enumerate(times):
                seg, d, basis = clock.scalars(t)
                host[f, 0] = np.array([seg], np.int32).view(np.float32)[0]
                host[f, 1] = d
                host[f, 2:14] = np.frombuffer(basis, dtype=np.float32, count=12)
            from .dynamics import _upload, _walk_order
            _walk_order(host)
            tab = _upload(host, self.dev)
            cache[key] = tab
        return tab

    def render_dynamic(self, clock, times, extr: Tensor, feature: Tensor, *, position: Tensor, pos_cubic_node: Tensor,
                       rotation: Tensor, rot_poly_feat: Tensor, rot_fourier_feat: Tensor, opacity: Tensor, scaling: Tensor,
                       cubic_layout: int = 1, bg: float = 0.0, nearest: float = 0.01, extent: float = 1.3,
                       grad_sink: Optional[Dict[str, Tensor]] = None, intr: Optional[Tensor] = None,
                       differentiable: bool = False, camera_grad: bool = False) -> Tensor:
        """images [F,C,H,W] of the reference's dynamic Gaussians (spline position, normalised rotation with the detached
        polynomial / Fourier sums, sigmoid opacity, exp scale: src/dynamic_gaussian_with_base_point_cloud.py:171-250) at the
        frame times ``times`` of ``clock``, evaluated inside the batched preprocess.  Differentiable w.r.t. position,
        pos_cubic_node, rotation, opacity, scaling and feature; ``grad_sink`` as in ``render``.

        ``differentiable=True`` (the opt-in of ``gs.alpha_blending_points``) opens the cameras of ``render_dynamic_sets``:
        ``extr`` [F,4,4] / [F,3,4] gives every frame its own camera and ``intr`` ([4] or [F,4]) selects the pinhole camera, with
        the same gradients; the cameras are constants (an ``extr`` / ``intr`` that requires grad raises).  One [4,4] camera is
        the path above, with its bits.  Without it ``extr`` is ONE camera and ``intr`` raises.

        ``camera_grad=True`` (needs ``differentiable=True``) makes the cameras leaves as well, as in ``render_dynamic_sets``."""
        self._forward_only_guard("render_dynamic", (position, pos_cubic_node, rotation, opacity, scaling, feature, extr, intr),
                                 bool(differentiable or camera_grad or grad_sink))
        tab = self.frame_table(clock, times)
        if camera_grad and not differentiable:
            raise ValueError("render_dynamic: camera_grad=True needs differentiable=True")
        cg = None
        if camera_grad:
            cg, cam, grad_sink = _camera_grad(extr, intr, grad_sink, self.F, "render_dynamic")
        sink = check_sink(grad_sink, {"position": position, "pos_cubic_node": pos_cubic_node, "rotation": rotation,
                                      "opacity": opacity, "scaling": scaling, "feature": feature})
        if intr is not None and not differentiable:
            raise ValueError("render_dynamic: intr= (the pinhole camera) needs differentiable=True")
        if cg is None:
            cam = _constant_camera(extr, intr, self.F, "render_dynamic") if differentiable else None
        return _RenderDynamic.apply(position, pos_cubic_node, rotation, opacity, scaling, feature, rot_poly_feat, rot_fourier_feat,
                                    (extr.detach() if cg is not None else extr) if cam is None else cam, tab, self,
                                    int(clock.interval_num), int(cubic_layout), float(bg), float(nearest), float(extent), sink,
                                    cg, extr if cg is not None else None, intr if cg is not None else None)

    def render_dynamic_sets(self, clock, times, extr: Tensor, sets, *, position: Tensor, pos_cubic_node: Tensor,
                            rotation: Tensor, rot_poly_feat: Tensor, rot_fourier_feat: Tensor, opacity: Tensor, scaling: Tensor,
                            cubic_layout: int = 1, K: int = 0, nearest: float = 0.01, extent: float = 1.3,
                            grad_sink: Optional[Dict[str, Tensor]] = None, points: Optional[dict] = None,
                            wide: Optional[dict] = None, intr: Optional[Tensor] = None, differentiable: bool = False,
                            camera_grad: bool = False):
        """The reference's real training frame, for all frames of the batch: its dynamic Gaussians (``render_dynamic``)
        through the three blends of ``render_iter`` (``render_sets``: same ``sets`` list, same return value).  The sets must
        fit the one-pass backward (one set per routing group, <= 4 / 4 / 20 channels).

        A set's ``feature`` may also be a LIST of tensors -- the set is their concatenation along the channels, as the
        reference's renderer concatenates its attributes (RenderFeatures.combine; ``["track_gs"] + render_attributes``,
        src/trainer_fragGS.py:511) -- and a tensor of a list may be per frame, ``[F, P, c]`` (track_gs = position(ids2) differs
        from frame to frame; a strided view with dense rows is read in place): no ``[F, P, C]`` row is materialised, a shared
        tensor's gradient is the sum over the frames, a per-frame tensor gets every frame's own.  ``grad_sink["feature:k"]``
        (k = position of the tensor in the flattened list of all sets' tensors) receives that gradient by ADDITION instead of
        autograd.  Any one-pass plan takes lists / per-frame tensors: the renderer's own plan (rgb 3 | depth 1 | 19 attribute
        channels) stages the forward's records in the tile kernel, other plans repack them in one launch.

        ``points``: one more feature set composited at SPARSE points only, outside the row (its channels do not count towards
        ``C``): a dict ``feature`` ([P, c] shared or [F, P, c] per frame), ``points`` [Q, 2] (float (ix, iy), the semantics of
        ``gs.alpha_blending_points``), ``offsets`` (device int64 [F + 1]: the queries offsets[f] .. offsets[f + 1] belong to frame
        f, as ``tracks.TrackTargets`` holds them), ``bg``, ``detach_opacity``.  The call then returns one more tensor [Q, c]
        behind the images and in front of ``gs_idx``, an output of the same autograd node: its gradient enters the batch's pair
        records between the tile backward and the Gaussian-side backward (float atomics: it raises in deterministic mode;
        ``ordered=True`` in the dict takes splat_alpha_blending_points_backward_batch_ordered instead: no float atomic, a fixed
        order of every sum, bit-reproducible and allowed in deterministic mode); the feature's gradient is ADDED to ``grad_sink["points"]`` (the feature's shape) when given, else returned through autograd.
        Not differentiable w.r.t. the points.  A ``None`` gradient of the sparse output launches nothing.

        ``wide``: one more DENSE feature set composited over the same sorted lists, outside the row (its channels do not count
        towards ``C``) -- render attributes wider than a one-pass plan holds, e.g. a 64-dimensional feature field
        (dptr_ortho_enhanced.py:361-376: the reference blends them with opacity.detach() in chunks of 32 channels): a dict
        ``feature`` ([P, c] float32 shared by the frames, any c >= 1), ``bg`` (default 0.0) and ``detach_opacity``, which must be
        True.  The call then returns one more tensor [F, c, H, W] behind the row's images and in front of the sparse output and
        ``gs_idx``, an output of the same autograd node.  Differentiable w.r.t. ``feature`` and, through uv / conic, the geometry
        parameters; not w.r.t. the opacity, and it feeds no taps.  Per 32-channel chunk its backward runs the tile kernels of the
        window and folds the chunk's records into the row's pair records before the Gaussian-side backward (no float atomics); the
        feature's gradient is ADDED to ``grad_sink["wide"]`` ([P, c]) when given, else returned through autograd.  A ``None``
        gradient of the wide output launches nothing.

        Cameras: ``extr`` [4,4] / [3,4] alone is the one orthographic camera of the video renderer -- the differentiable path
        above.  ``extr`` [F,4,4] / [F,3,4] gives every frame its own camera (a novel-view orbit, the two eyes of a stereo clip)
        and ``intr`` ((fx, fy, cx, cy), [4] or [F,4], as in ``render_sets``) selects the pinhole camera.  Per-frame and pinhole
        cameras of a dynamic batch are FORWARD ONLY by default: the same tuple comes back with nothing requiring grad (``K``,
        ``wide`` as above); under grad mode with a parameter or feature that requires grad the call raises, and so does
        ``points=``.

        ``differentiable=True`` (the opt-in of ``gs.alpha_blending_points``) trains under these cameras: the same autograd node
        as the one-camera path, with the batched forward under the cameras and, behind the unchanged tile backward, the
        Gaussian-side backward of include/splat_hip_views_grad.h -- every frame's records go back through that frame's camera.
        Everything the one-camera path takes it takes (``grad_sink``, feature lists and per-frame tensors, ``K``, ``wide``,
        ``points`` with ``ordered`` and the deterministic-mode rule).  The cameras are constants: an ``extr`` / ``intr`` that
        requires grad raises instead of being detached.  One [4,4] camera with ``differentiable=True`` is the path above.

        ``camera_grad=True`` (needs ``differentiable=True``) makes the cameras leaves of the same autograd node: ``extr`` ([4,4] /
        [3,4] / [F,4,4] / [F,3,4]) and ``intr`` ([4] / [F,4]) may require grad and receive gradients of their own shape -- zeros in
        the bottom row of a 4x4, the sum over the frames for a camera the frames share -- or ``grad_sink["extr"]`` /
        ``grad_sink["intr"]`` (float32 GPU buffers of the tensor's shape) receive them by ADDITION.  Behind the tile, sparse and
        wide backward one more kernel sums the pair records per frame under that frame's camera
        (include/splat_hip_camera_grad.h: orthographic cameras, per frame or one, and the pinhole camera; no float atomics,
        bit-reproducible, allowed in deterministic mode); the parameter and feature gradients keep their bits, and a camera
        that neither requires grad nor has a sink launches nothing.  ``views.pose_delta`` is the parameterisation a pose
        refinement optimises.  Not differentiated: the cull / near / extent decisions and the radius."""
        self._forward_only_guard("render_dynamic_sets", [position, pos_cubic_node, rotation, opacity, scaling, extr, intr]
                                 + _set_tensors(sets, points, wide), bool(differentiable or camera_grad or grad_sink))
        tab = self.frame_table(clock, times)
        cam = dcam = cg = None
        if camera_grad:
            if not differentiable:
                raise ValueError("render_dynamic_sets: camera_grad=True needs differentiable=True")
            cg, dcam, grad_sink = _camera_grad(extr, intr, grad_sink, self.F, "render_dynamic_sets")
        elif differentiable:
            dcam = _constant_camera(extr, intr, self.F, "render_dynamic_sets")
        elif intr is not None or (isinstance(extr, Tensor) and extr.dim() == 3):
            cam = _Camera(extr.detach(), None if intr is None else intr.detach(), self.F)
            if points is not None:
                raise ValueError("render_dynamic_sets: points= is not built for per-frame and pinhole cameras of a dynamic batch")
            if grad_sink:
                raise ValueError("render_dynamic_sets: per-frame and pinhole cameras of a dynamic batch are forward only "
                                 "(grad_sink has no backward to feed)")
        meta, parts, feats = _parse_sets(sets, self.F, self.P)
        widths = [1 if m[0] == "depth" else m[0] for m in meta]
        if sum(widths) != self.C:
            raise ValueError(f"the sets hold {sum(widths)} channels, the batch was built for C = {self.C}")
        plan = _one_pass_plan(meta, widths, self.C)
        if plan is None:
            raise ValueError("render_dynamic_sets needs sets that fit the one-pass backward: one set per routing group "
                             "(taps / live opacity / detached opacity) of at most 4 / 4 / 20 channels")
        fsink = {k: v for k, v in (grad_sink or {}).items() if k.startswith("feature:")}
        psink = {k: v for k, v in (grad_sink or {}).items() if not k.startswith("feature:") and k not in ("points", "wide")}
        pts = _parse_points(points, (grad_sink or {}).get("points"), self.F, self.P)
        if pts is None and "points" in (grad_sink or {}):
            raise ValueError('grad_sink["points"] belongs to the sparse set: pass points=...')
        wd = _parse_wide(wide, (grad_sink or {}).get("wide"), self.P)
        sink = check_sink(psink, {"position": position, "pos_cubic_node": pos_cubic_node, "rotation": rotation,
                                  "opacity": opacity, "scaling": scaling})
        for k, buf in fsink.items():
            i = int(k.split(":")[1])
            if not (0 <= i < len(feats)) or tuple(buf.shape) != tuple(feats[i].shape) or buf.dtype != torch.float32 \
                    or not buf.is_cuda or buf.stride(-1) != 1 or buf.stride(-2) != buf.shape[-1]:
                raise ValueError(f"grad_sink[{k!r}] must be a float32 GPU buffer of the feature tensor's shape with dense rows")
        if cam is not None:
            every = [position, pos_cubic_node, rotation, opacity, scaling] + list(feats) + ([wide["feature"]] if wd is not None else [])
            if torch.is_grad_enabled() and any(isinstance(t, Tensor) and t.requires_grad for t in every):
                raise ValueError("render_dynamic_sets: per-frame and pinhole cameras of a dynamic batch are forward only (the "
                                 "Gaussian-side backward under these cameras is not built); call it under torch.no_grad() or "
                                 "with detached tensors")
            with torch.no_grad():
                st = _dynamic_sets_forward(self, position, pos_cubic_node, rotation, opacity, scaling, rot_poly_feat,
                                           rot_fourier_feat, cam, tab, int(clock.interval_num), int(cubic_layout), meta,
                                           int(K), float(nearest), float(extent), parts, None, wd,
                                           tuple(feats) + ((wide["feature"],) if wd is not None else ()))
            return st["outputs"]
        return _RenderDynamicSets.apply(position, pos_cubic_node, rotation, opacity, scaling, rot_poly_feat, rot_fourier_feat,
                                        (extr.detach() if cg is not None else extr) if dcam is None else dcam, tab, self,
                                        int(clock.interval_num), int(cubic_layout), meta, int(K), float(nearest),
                                        float(extent), sink, parts, fsink or None, pts, wd,
                                        cg, extr if cg is not None else None, intr if cg is not None else None,
                                        *(list(feats) + ([pts["feature"]] if pts is not None else [])
                                          + ([wide["feature"]] if wd is not None else [])))

    # ------------------------------------------------------------------ several feature sets of one geometry (row a1)
    def render_sets(self, xyz: Tensor, scales: Tensor, uquats: Tensor, opacity: Tensor, sets, offsets: Optional[Tensor],
                    extr: Tensor, K: int = 0, nearest: float = 0.01, extent: float = 1.3,
                    grad_sink: Optional[Dict[str, Tensor]] = None, intr: Optional[Tensor] = None, wide: Optional[dict] = None):
        """The reference renderer's blends of ONE geometry over all frames of the batch (render_iter,
        src/pointrix/renderer/dptr_ortho_enhanced.py:331-375: rgb through alpha_blending_enhanced with the taps; depth with
        bg = 1; the extra attributes with opacity.detach()).  ``sets``: a list of dicts ``feature`` ([P,c] tensor shared by
        the frames, or the string "depth" for the per-frame depth of the projection), ``bg``, ``detach_opacity``, ``taps``.
        The widths must add up to the batch's ``C``.  One forward pass composites the concatenated row; per set one
        backward pass of the tile kernels and one Gaussian-side reduction.  Returns ``(images per set ..., gs_idx)`` with
        images [F,c,H,W] and gs_idx [F,H,W,K] (None for K = 0).  Cameras (``extr`` per frame, ``intr``) as in ``render``.
        ``wide``: one more detached feature set of any width outside the row, as in ``render_dynamic_sets`` (its image [F,c,H,W]
        comes behind the sets' images, in front of ``gs_idx``; ``grad_sink["wide"]``); the sets must then fit the one-pass
        backward."""
        self._forward_only_guard("render_sets", [xyz, scales, uquats, opacity, offsets] + _set_tensors(sets, None, wide),
                                 bool(grad_sink))
        def one(f):
            # a list of shared tensors = their concatenation along the channels, as the reference's renderer concatenates its
            # attributes (RenderFeatures.combine); per-frame tensors belong to the dynamic renderer (render_dynamic_sets)
            if isinstance(f, (list, tuple)):
                if any(t.dim() != 2 for t in f):
                    raise ValueError("render_sets: the tensors of a feature list are [P, c] (per-frame tensors: render_dynamic_sets)")
                return f[0] if len(f) == 1 else torch.cat(list(f), dim=1)
            return f
        sets = [dict(s_, feature=one(s_["feature"])) for s_ in sets]
        feats = [s_["feature"] for s_ in sets if not isinstance(s_["feature"], str)]
        meta = tuple((("depth" if isinstance(s_["feature"], str) else int(s_["feature"].shape[1])), float(s_.get("bg", 0.0)),
                      bool(s_.get("detach_opacity", False)), bool(s_.get("taps", False))) for s_ in sets)
        width = sum(1 if m[0] == "depth" else m[0] for m in meta)
        if width != self.C:
            raise ValueError(f"the sets hold {width} channels, the batch was built for C = {self.C}")
        if sum(1 for m in meta if m[3]) > 1:
            raise ValueError("at most one set feeds the densification taps")
        wd = _parse_wide(wide, (grad_sink or {}).get("wide"), self.P)
        if wd is not None:
            grad_sink = {k: v for k, v in (grad_sink or {}).items() if k != "wide"} or None
            if not OPTIONS["sets_one_pass"] or _one_pass_plan(meta, [1 if m[0] == "depth" else m[0] for m in meta], self.C) is None:
                raise ValueError("render_sets(wide=...) needs sets that fit the one-pass backward: one set per routing group "
                                 "(taps / live opacity / detached opacity) of at most 4 / 4 / 20 channels")
            feats = feats + [wide["feature"]]
        sink = check_sink(grad_sink, {"xyz": xyz, "scales": scales, "uquats": uquats, "opacity": opacity})
        res = _RenderSets.apply(xyz, scales, uquats, opacity, offsets, extr, self, meta, int(K), float(nearest), float(extent),
                                sink, intr, wd, *feats)
        return res


def _args_of(forward, *leaves) -> tuple:
    """the argument table of an autograd node: the names of its ``forward``'s parameters behind ``ctx`` (a ``*feats`` last, so that
    ``index("feats")`` is the number of fixed arguments), read ONCE, at import.  Every position and every ``None`` padding of the
    node's ``backward`` comes from this table: an argument added to a ``forward`` moves them with it.  ``leaves``: the
    differentiable parameters, which lead the table in this order (a ``backward`` returns their gradients first)."""
    names = tuple(inspect.signature(forward.__func__).parameters)[1:]
    assert names[:len(leaves)] == leaves, (names, leaves)
    return names


def _entry(name: str, cam: Optional[_Camera], extr: Tensor):
    """an entry point that takes a camera, and its camera argument: the core header's ``name`` with the 12 floats ``extr`` of the
    one orthographic camera when ``cam`` is None, else its ``_cam`` twin (include/splat_hip_views.h, splat_hip_views_grad.h,
    splat_hip_layers_cam.h) with the ``_Camera``'s struct"""
    if cam is None:
        return getattr(L.lib(), name), L.ptr(extr)
    return getattr(L.lib(), name + "_cam"), ctypes.byref(cam.struct())


def _backward_entry(ctx, name: str, extr_c: Tensor):
    """``_entry`` for the Gaussian-side backward of a dynamic batch: it re-reads the forward's cameras through raw pointers, so
    they must not have been edited in place since"""
    if ctx.cam is not None:
        _check_versions(ctx.cam_versions, "a camera tensor")
    return _entry(name, ctx.cam, extr_c)


def _dynamic_geometry(fb, position, cubic, rotation, opacity, scaling, rot_poly, rot_fourier, extr, tab, I, layout, nearest, extent):
    """the geometry of a dynamic batch's forward: the raw parameters normalised and checked against the batch, the batched dynamic
    preprocess (splat_frame_preprocess_forward_batch[_cam]) under ``extr`` -- the tensor of the one orthographic camera, or a
    ``_Camera`` (cameras per frame / the pinhole camera) --, tile binning and sort.  Returns (the seven normalised parameters in the order of the arguments, ``opa_t`` [P, 1]:
    the activated opacity, ``extr_c``: the camera tensor a backward saves, the generation of this forward)."""
    P = fb.P
    position = _points(position, "position", 3)
    rotation = _points(rotation, "rotation", 4)
    scaling = _points(scaling, "scaling", 3)
    opacity = L.need(opacity, "opacity")
    cubic = L.need(cubic, "pos_cubic_node")
    rot_poly, rot_fourier = L.need(rot_poly, "rot_poly_feat"), L.need(rot_fourier, "rot_fourier_feat")
    if cubic.numel() != P * 4 * I * 3 or rot_poly.numel() != P * 16 or rot_fourier.numel() != P * 32 or opacity.numel() != P:
        raise ValueError("parameter shapes do not match the batch (P Gaussians, I spline segments)")
    if position.shape[0] != P or rotation.shape[0] != P or scaling.shape[0] != P:
        raise ValueError(f"the batch was built for {P} Gaussians")
    cam = extr if isinstance(extr, _Camera) else None
    extr_c = _extr12(extr) if cam is None else cam.extr
    gen = fb._begin_forward()
    opa_t = torch.empty(P, 1, dtype=torch.float32, device=fb.dev)
    preprocess, cam_arg = _entry("splat_frame_preprocess_forward_batch", cam, extr_c)
    L.check(preprocess(
        fb.F, P, I, L.ptr(tab), L.ptr(position), L.ptr(cubic), layout, L.ptr(rotation), L.ptr(rot_poly),
        L.ptr(rot_fourier), L.ptr(opacity), L.ptr(scaling), cam_arg, fb.W, fb.H, nearest, extent,
        L.ptr(fb.uv), L.ptr(fb.depth), L.ptr(fb.conic), L.ptr(fb.radius), L.ptr(opa_t), L.stream()))
    fb._bin_and_sort(opa_t)
    return (position, cubic, rotation, opacity, scaling, rot_poly, rot_fourier), opa_t, extr_c, gen


class _RenderDynamic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, position, cubic, rotation, opacity, scaling, feature, rot_poly, rot_fourier, extr, tab, fb, I, layout, bg,
                nearest, extent, sink, cg=None, cg_extr=None, cg_intr=None):
        F, P, W, H, C = fb.F, fb.P, fb.W, fb.H, fb.C
        ctx.cg = cg                                           # camera_grad=True: cg_extr / cg_intr are the camera leaves
        feature = _points(feature, "feature", C)
        if feature.shape[0] != P:
            raise ValueError(f"the batch was built for {P} Gaussians")
        (position, cubic, rotation, opacity, scaling, rot_poly, rot_fourier), opa_t, extr_c, ctx.gen = _dynamic_geometry(
            fb, position, cubic, rotation, opacity, scaling, rot_poly, rot_fourier, extr, tab, I, layout, nearest, extent)
        ctx.cam = cam = extr if isinstance(extr, _Camera) else None     # cameras per frame / the pinhole camera (differentiable=True)
        ctx.cam_versions = _versions(*cam.tensors()) if cam is not None else ()
        out = torch.empty(F, C, H, W, dtype=torch.float32, device=fb.dev)
        L.check(L.lib().splat_alpha_blending_forward_batch(
            F, P, C, L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(opa_t), 0, L.ptr(feature),
            0, L.ptr(fb.idx_sorted), L.ptr(fb.tile_range), fb.capacity, bg, L.ptr(None), W,
            H, 0, 0, L.ptr(out), L.ptr(fb.final_T), L.ptr(fb.ncontrib), L.ptr(None), L.ptr(fb.pack),
            L.ptr(fb.cull_flags), L.stream()))
        ctx.fb, ctx.meta, ctx.sink = fb, (I, layout, bg), sink
        ctx.save_for_backward(position, cubic, rotation, opacity, scaling, feature, rot_poly, rot_fourier, extr_c, tab)
        return out

    ARGS = _args_of(forward, "position", "cubic", "rotation", "opacity", "scaling", "feature")
    CG_EXTR, CG_INTR = ARGS.index("cg_extr"), ARGS.index("cg_intr")

    @staticmethod
    def backward(ctx, dL_dout):
        A, fb = _RenderDynamic, ctx.fb
        fb._check_generation(ctx.gen)
        position, cubic, rotation, opacity, scaling, feature, rot_poly, rot_fourier, extr_c, tab = ctx.saved_tensors
        I, layout, bg = ctx.meta
        sink, nig = ctx.sink or {}, ctx.needs_input_grad
        g = L.need(dL_dout, "dL_dout")
        lib, st = L.lib(), L.stream()
        F, P, W, H, C, cap = fb.F, fb.P, fb.W, fb.H, fb.C, fb.capacity
        from .gs.raster_ops import _debug_T_front
        L.check(lib.splat_alpha_blending_backward_batch(
            F, P, C, L.ptr(fb.idx_sorted), L.ptr(fb.tile_range), cap, bg, W, H,
            L.ptr(fb.final_T), L.ptr(fb.ncontrib), L.ptr(g), 1 if fb.want_abs else 0, L.ptr(fb.slot_sorted),
            L.ptr(fb.pair_records), L.ptr(fb.pack), L.ptr(fb.cull_flags), L.ptr(_debug_T_front(F * H, W, g.device)), st))
        like = {"position": position, "pos_cubic_node": cubic, "rotation": rotation, "opacity": opacity, "scaling": scaling,
                "feature": feature}
        need = dict(zip(like, nig))                           # (the leaves lead the argument table)
        bufs = {k: (sink[k] if k in sink else (torch.zeros_like(v) if need[k] else None)) for k, v in like.items()}
        gauss_backward, cam_arg = _backward_entry(ctx, "splat_frames_gauss_backward_dynamic", extr_c)
        L.check(gauss_backward(
            F, P, I, C, W, H, cap, 1 if fb.want_abs else 0,
            L.ptr(fb.pair_records), L.ptr(fb.goff), L.ptr(fb.radius), L.ptr(tab), L.ptr(position), L.ptr(cubic), layout,
            L.ptr(rotation), L.ptr(rot_poly), L.ptr(rot_fourier), L.ptr(opacity), L.ptr(scaling), cam_arg,
            L.ptr(bufs["position"]), L.ptr(bufs["pos_cubic_node"]), L.ptr(bufs["rotation"]), L.ptr(bufs["opacity"]),
            L.ptr(bufs["scaling"]), L.ptr(bufs["feature"]), L.ptr(fb.tap), L.ptr(fb.abs_tap), L.ptr(fb.radii_max), st))
        ret = [None] * len(A.ARGS)
        ret[:len(like)] = [None if k in sink else bufs[k] for k in like]
        if ctx.cg is not None:
            ret[A.CG_EXTR], ret[A.CG_INTR] = ctx.cg.backward(
                fb, fb.pair_records, fb.ncp, -1, tab, position, cubic, layout, I, rotation, rot_poly, rot_fourier, scaling,
                nig[A.CG_EXTR], nig[A.CG_INTR])
        return tuple(ret)


def _dynamic_sets_forward(fb, position, cubic, rotation, opacity, scaling, rot_poly, rot_fourier, extr, tab, I, layout, meta,
                          K, nearest, extent, parts, pts, wd, feats):
    """the forward of ``render_dynamic_sets``: the dynamic geometry (``_dynamic_geometry``), the sets' blends, the wide and the
    sparse set.  ``extr``: the tensor of the one orthographic camera (the differentiable path: ``_RenderDynamicSets``), or a
    ``_Camera``: cameras per frame and / or the pinhole camera (forward only by default; ``_RenderDynamicSets`` with a
    ``_Camera`` is the differentiable path under them)."""
    P, F = fb.P, fb.F
    pfeat = wfeat = None
    if wd is not None:        # the wide set's feature rides last
        feats, wfeat = feats[:-1], L.need(feats[-1], "wide feature")
    if pts is not None:       # the sparse set's feature rides behind the sets' tensors
        feats, pfeat = feats[:-1], feats[-1]
    sources = _has_sources(parts)
    if not sources:
        _check_set_features(meta, feats, P)
    geo, opa_t, extr_c, gen = _dynamic_geometry(fb, position, cubic, rotation, opacity, scaling, rot_poly, rot_fourier, extr, tab,
                                                I, layout, nearest, extent)
    if sources:
        feats = tuple(_source_tensor(t, pf, F, P) for t, (_, pf) in zip(feats, [p_ for pp in parts for p_ in pp]))
        out, gs_idx, blend = _blend_sources_forward(fb, meta, parts, feats, opa_t, K)
    else:
        out, gs_idx, blend = _blend_sets_forward(fb, meta, feats, opa_t, 0, K)
    if blend["plan"] is None:
        raise ValueError("render_dynamic_sets needs sets that fit the one-pass backward")
    sparse = ()
    if pts is not None:
        pfeat = _source_tensor(pfeat, pts["per_frame"], F, P)
        sparse = (_points_forward(fb, pts, pfeat, opa_t),)
        feats = tuple(feats) + (pfeat,)
    wide_out = ()
    if wd is not None:
        wide_out = (_wide_forward(fb, wd, wfeat, opa_t, 0),)
        feats = tuple(feats) + (wfeat,)
    return dict(gen=gen, blend=blend, sources=sources, opa_t=opa_t, saved=geo + (extr_c, tab) + tuple(feats),
                outputs=tuple(_split_row(out, meta)) + wide_out + sparse + (gs_idx,))


def _split_row(out: Tensor, meta) -> list:
    """the composited row [F, C, H, W] by the sets' widths: one image [F, c, H, W] per set (views)"""
    imgs, c0 = [], 0
    for w, _, _, _ in meta:
        w = 1 if w == "depth" else w
        imgs.append(out[:, c0:c0 + w])
        c0 += w
    return imgs


def _side_backward(wanted: bool, sink: Optional[Tensor], feature: Tensor, run) -> tuple:
    """the backward of a set beside the row (the wide set, the sparse set) whose output received a gradient: ``run(buffer)`` puts
    its geometry terms into the pair records and ADDS its feature's gradient to ``buffer`` -- the ``sink``, else zeros of the
    feature's shape when autograd wants it (``wanted``), else None.  Returns the 1-tuple for autograd: a sink keeps its
    gradient from it."""
    buf, ret = sink, None
    want = wanted or sink is not None
    if want and buf is None:
        buf = ret = torch.zeros(feature.shape, dtype=torch.float32, device=feature.device)
    run(buf if want else None)
    return (ret,)


def _group_grads(meta, plan, feats, grads, wanted):
    """the feature gradients of a one-pass plan whose sets are one tensor each: (per tensor zeros of its shape, or None where its
    set received no gradient or autograd does not want it (``wanted``: per tensor); the ``c0 / cn / d_feature / stride`` arguments
    of the three routing groups for the Gaussian-side entry points)"""
    group_of = _set_groups(meta)
    fi, dfe, dfs, strides = 0, [], [0, 0, 0], [0, 0, 0]
    for si, (w, _, _, _) in enumerate(meta):
        if w == "depth":
            continue
        dfeat = torch.zeros_like(feats[fi]) if grads[si] is not None and wanted[fi] else None
        dfe.append(dfeat)
        dfs[group_of[si]], strides[group_of[si]] = (0 if dfeat is None else dfeat.data_ptr()), int(feats[fi].shape[1])
        fi += 1
    i3 = ctypes.c_int32 * 3
    return tuple(dfe), (i3(*plan[0]), i3(*plan[1]), (ctypes.c_void_p * 3)(*dfs), i3(*strides))


def _source_grads(meta, parts, feats, grads, wanted, fsink):
    """the feature gradients of a row by SOURCES -- a shared tensor's is the sum over the frames, a per-frame tensor gets every
    frame's own --: (per tensor zeros of its shape for autograd, or None; the ``n, table`` arguments of the Gaussian-side entry
    point: the sources whose gradient autograd (``wanted``: per tensor) or a ``grad_sink["feature:k"]`` buffer receives)"""
    table = (L.FeatureSource * L.MAX_SOURCES)()
    dfe, n, fi, c0 = [], 0, 0, 0
    for si, ((w, _, _, _), pp) in enumerate(zip(meta, parts)):
        if w == "depth":
            c0 += 1
            continue
        for cn, per_frame in pp:
            t, buf, ret = feats[fi], fsink.get(f"feature:{fi}"), None
            need = grads[si] is not None and (wanted[fi] or buf is not None)
            if need and buf is None:
                buf = ret = torch.zeros(t.shape, dtype=torch.float32, device=t.device)
            dfe.append(ret)
            if need:
                table[n].c0, table[n].cn, table[n].feature = c0, cn, t.data_ptr()
                table[n].d_feature = buf.data_ptr()
                table[n].frame_stride = int(buf.stride(0)) if per_frame else 0
                n += 1
            c0 += cn
            fi += 1
    return tuple(dfe), (n, table)


class _RenderDynamicSets(torch.autograd.Function):
    @staticmethod
    def forward(ctx, position, cubic, rotation, opacity, scaling, rot_poly, rot_fourier, extr, tab, fb, I, layout, meta, K,
                nearest, extent, sink, parts, fsink, pts, wd, cg, cg_extr, cg_intr, *feats):
        ctx.cg = cg                                           # camera_grad=True: cg_extr / cg_intr are the camera leaves
        st = _dynamic_sets_forward(fb, position, cubic, rotation, opacity, scaling, rot_poly, rot_fourier, extr, tab, I, layout,
                                   meta, K, nearest, extent, parts, pts, wd, feats)
        ctx.cam = cam = extr if isinstance(extr, _Camera) else None     # cameras per frame / the pinhole camera (differentiable=True)
        ctx.cam_versions = _versions(*cam.tensors()) if cam is not None else ()
        ctx.gen, ctx.blend = st["gen"], st["blend"]
        ctx.fb, ctx.meta, ctx.sink, ctx.geo = fb, meta, sink, (I, layout)
        ctx.parts, ctx.fsink, ctx.sources = parts, (fsink or {}), st["sources"]
        ctx.opa_t = st["opa_t"]
        ctx.pts = pts
        ctx.wd = wd
        ctx.save_for_backward(*st["saved"])
        ctx.set_materialize_grads(False)
        if st["outputs"][-1] is not None:
            ctx.mark_non_differentiable(st["outputs"][-1])
        return st["outputs"]

    ARGS = _args_of(forward, "position", "cubic", "rotation", "opacity", "scaling")
    CG_EXTR, CG_INTR, FEATS = ARGS.index("cg_extr"), ARGS.index("cg_intr"), ARGS.index("feats")

    @staticmethod
    def backward(ctx, *grads):
        A, fb = _RenderDynamicSets, ctx.fb
        fb._check_generation(ctx.gen)
        position, cubic, rotation, opacity, scaling, rot_poly, rot_fourier, extr_c, tab = ctx.saved_tensors[:9]
        feats = ctx.saved_tensors[9:]
        meta, sink, nig = ctx.meta, (ctx.sink or {}), ctx.needs_input_grad
        I, layout = ctx.geo
        F, P, W, H, C, cap = fb.F, fb.P, fb.W, fb.H, fb.C, fb.capacity
        pts, pfeat, g_pts = ctx.pts, None, None
        wd, wfeat, g_wide = ctx.wd, None, None
        if wd is not None:
            feats, wfeat = feats[:-1], feats[-1]
            g_wide = grads[len(meta)]
        if pts is not None:
            feats, pfeat = feats[:-1], feats[-1]
            g_pts = grads[len(meta) + (1 if wd is not None else 0)]
        like = {"position": position, "pos_cubic_node": cubic, "rotation": rotation, "opacity": opacity, "scaling": scaling}
        bufs = {k: (sink[k] if k in sink else torch.zeros_like(v)) for k, v in like.items()}
        plan = _one_pass_plan(meta, ctx.blend["widths"], C)
        depth_ch, has_tap = plan[3], plan[4] is not None
        want_abs = 1 if (has_tap and fb.want_abs) else 0
        wanted = nig[A.FEATS:]                                # per feature tensor: the sets' tensors, the sparse, the wide set's
        # the sets' tensors: by SOURCES (a feature list, a per-frame tensor), or one tensor per routing group -- two entry points
        # that differ in these arguments alone
        if ctx.sources:
            name, (dfe, features) = "splat_frames_gauss_backward_dynamic_sources", _source_grads(meta, ctx.parts, feats, grads, wanted,
                                                                                                   ctx.fsink)
        else:
            name, (dfe, features) = "splat_frames_gauss_backward_dynamic_sets", _group_grads(meta, plan, feats, grads, wanted)
        rec = _blend_sets_backward_one_pass(fb, meta, ctx.blend, grads[:len(meta)], ctx.opa_t, 0, want_abs)
        # the sparse, then the wide set: into the pair records the tile backward has just written, before the Gaussian-side walk
        d_pts = () if pts is None else (None,) if g_pts is None else _side_backward(
            wanted[len(feats)], pts["sink"], pfeat, lambda buf: _points_backward(fb, pts, pfeat, ctx.opa_t, g_pts, rec, buf))
        d_wide = () if wd is None else (None,) if g_wide is None else _side_backward(
            wanted[len(feats) + len(d_pts)], wd["sink"], wfeat, lambda buf: _wide_backward(fb, wd, wfeat, ctx.opa_t, 0, g_wide, rec, buf))
        gauss_backward, cam_arg = _backward_entry(ctx, name, extr_c)
        L.check(gauss_backward(
            F, P, I, C, W, H, cap, L.ptr(rec), L.ptr(fb.goff), L.ptr(fb.radius),
            L.ptr(tab), L.ptr(position), L.ptr(cubic), layout, L.ptr(rotation), L.ptr(rot_poly), L.ptr(rot_fourier),
            L.ptr(opacity), L.ptr(scaling), cam_arg, L.ptr(bufs["position"]), L.ptr(bufs["pos_cubic_node"]),
            L.ptr(bufs["rotation"]), L.ptr(bufs["opacity"]), L.ptr(bufs["scaling"]), *features,
            depth_ch, L.ptr(fb.tap if has_tap else None), L.ptr(fb.abs_tap if (has_tap and want_abs) else None),
            L.ptr(fb.radii_max if has_tap else None), L.stream()))
        ret = [None] * A.FEATS
        ret[:len(like)] = [None if k in sink else bufs[k] for k in like]
        if ctx.cg is not None:        # the camera leaves (camera_grad=True): from the records every backward above has filled
            ret[A.CG_EXTR], ret[A.CG_INTR] = ctx.cg.backward(
                fb, rec, int(L.lib().splat_blend_sets_pair_stride(C)), 12 + depth_ch if depth_ch >= 0 else -1, tab, position, cubic,
                layout, I, rotation, rot_poly, rot_fourier, scaling, nig[A.CG_EXTR], nig[A.CG_INTR])
        return tuple(ret) + dfe + d_pts + d_wide


def _parse_points(points, sink, F, P):
    """the sparse set of ``render_dynamic_sets``: None, or its checked description (feature, points [Q,2], offsets [F+1], bg,
    detach_opacity, per_frame, the feature's gradient sink or None); nothing here reads device memory"""
    if points is None:
        return None
    unknown = set(points) - {"feature", "points", "offsets", "bg", "detach_opacity", "ordered"}
    if unknown:
        raise ValueError(f"points: unknown keys {sorted(unknown)}")
    f, xy, off = points.get("feature"), points.get("points"), points.get("offsets")
    if not isinstance(f, Tensor) or f.dim() not in (2, 3) or f.shape[-2] != P or (f.dim() == 3 and f.shape[0] != F) \
            or f.shape[-1] < 1 or f.dtype != torch.float32 or not f.is_cuda:
        raise ValueError(f"points['feature'] must be a float32 GPU tensor [P={P}, c] or [F={F}, P, c]")
    if not isinstance(xy, Tensor) or xy.dim() != 2 or xy.shape[1] != 2:
        raise ValueError("points['points'] must be [Q, 2] (ix, iy)")
    if xy.requires_grad:
        raise ValueError("the sparse set is not differentiable w.r.t. its points")
    if not isinstance(off, Tensor) or off.dtype != torch.int64 or tuple(off.shape) != (F + 1,) or not off.is_cuda:
        raise ValueError(f"points['offsets'] must be a device int64 tensor [F + 1 = {F + 1}]")
    if sink is not None and (tuple(sink.shape) != tuple(f.shape) or sink.dtype != torch.float32 or not sink.is_cuda
                             or sink.stride(-1) != 1 or sink.stride(-2) != sink.shape[-1]):
        raise ValueError('grad_sink["points"] must be a float32 GPU buffer of the sparse feature\'s shape with dense rows')
    return dict(feature=f, points=L.need(xy.detach(), "points"), offsets=L.need(off, "offsets", torch.int64),
                bg=float(points.get("bg", 0.0)), detach_opacity=bool(points.get("detach_opacity", False)),
                ordered=bool(points.get("ordered", False)), per_frame=f.dim() == 3, sink=sink)


def _points_forward(fb, pts, pfeat, opacity):
    """the sparse set at its points (splat_alpha_blending_points_forward_batch on the batch's buffers): [Q, c]; the corners'
    final transmittance / last applied position stay in ``pts`` for the backward"""
    Q, c = int(pts["points"].shape[0]), int(pfeat.shape[-1])
    out = torch.empty(Q, c, dtype=torch.float32, device=fb.dev)
    pts["corner_T"] = torch.empty(Q, 4, dtype=torch.float32, device=fb.dev)
    pts["corner_n"] = torch.empty(Q, 4, dtype=torch.int32, device=fb.dev)
    L.check(L.lib().splat_alpha_blending_points_forward_batch(
        fb.F, fb.P, c, L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(opacity), 0, L.ptr(pfeat),
        int(pfeat.stride(0)) if pts["per_frame"] else 0, L.ptr(fb.idx_sorted), L.ptr(fb.tile_range),
        fb.capacity, pts["bg"], fb.W, fb.H, Q, L.ptr(pts["offsets"]),
        L.ptr(pts["points"]), L.ptr(out), L.ptr(pts["corner_T"]), L.ptr(pts["corner_n"]), L.stream()))
    return out


def _points_backward(fb, pts, pfeat, opacity, g, rec, d_feature):
    """splat_alpha_blending_points_backward_batch: the sparse set's geometry gradients into the SETS pair records ``rec`` the tile
    backward has written, its feature gradient added to ``d_feature`` (the feature's shape; None: not wanted)"""
    Q, c = int(pts["points"].shape[0]), int(pfeat.shape[-1])
    g = L.need(g, "gradient of the sparse output")
    if tuple(g.shape) != (Q, c):
        raise ValueError(f"the gradient of the sparse output must be [{Q}, {c}]")
    dfs = 0 if d_feature is None or not pts["per_frame"] else int(d_feature.stride(0))
    lib, name, tail = L.lib(), "splat_alpha_blending_points_backward_batch", ()
    if pts["ordered"]:
        # no float atomic, every sum in a fixed order (runs in deterministic mode too): the batch's pair map and a pooled scratch
        need = int(lib.splat_alpha_blending_points_backward_batch_ordered_scratch_bytes(fb.F, c, fb.W, fb.H, Q, fb.capacity))
        if need == 0:
            raise ValueError("the ordered sparse backward: sizes too large")
        scratch = fb._set_buffer(("points", "ordered"), (need + 3) // 4)
        name, tail = name + "_ordered", (L.ptr(fb.goff), L.ptr(scratch), scratch.numel() * 4)
    L.check(getattr(lib, name)(
        fb.F, fb.P, c, L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(opacity), 0, L.ptr(pfeat),
        int(pfeat.stride(0)) if pts["per_frame"] else 0, L.ptr(fb.idx_sorted), L.ptr(fb.tile_range),
        fb.capacity, pts["bg"], fb.W, fb.H, Q, L.ptr(pts["offsets"]),
        L.ptr(pts["points"]), L.ptr(pts["corner_T"]), L.ptr(pts["corner_n"]), L.ptr(g), L.ptr(fb.slot_sorted), L.ptr(rec),
        int(lib.splat_blend_sets_pair_stride(fb.C)), 1 if pts["detach_opacity"] else 0, L.ptr(d_feature),
        dfs, *tail, L.stream()))


def _parse_wide(wide, sink, P):
    """the wide detached set of ``render_sets`` / ``render_dynamic_sets``: None, or its checked description (feature [P, c], bg,
    the feature's gradient sink or None); nothing here reads device memory"""
    if wide is None:
        if sink is not None:
            raise ValueError('grad_sink["wide"] belongs to the wide set: pass wide=...')
        return None
    if not isinstance(wide, dict):
        raise ValueError("wide: a dict feature / bg / detach_opacity")
    unknown = set(wide) - {"feature", "bg", "detach_opacity"}
    if unknown:
        raise ValueError(f"wide: unknown keys {sorted(unknown)}")
    if wide.get("detach_opacity") is not True:
        raise ValueError("wide: detach_opacity must be True (the reference blends its render attributes with opacity.detach(); "
                         "a set blended with the live opacity belongs in the row)")
    f = wide.get("feature")
    if not isinstance(f, Tensor) or f.dim() != 2 or f.shape[0] != P or f.shape[1] < 1 or f.dtype != torch.float32:
        raise ValueError(f"wide['feature'] must be a float32 tensor [P={P}, c] with c >= 1, shared by the frames")
    if not f.is_cuda:
        raise ValueError("wide['feature'] must be a CUDA (ROCm) tensor (there is no CPU path)")
    if sink is not None and (not isinstance(sink, Tensor) or tuple(sink.shape) != tuple(f.shape) or sink.dtype != torch.float32
                             or not sink.is_cuda or not sink.is_contiguous()):
        raise ValueError('grad_sink["wide"] must be a contiguous float32 GPU buffer of the wide feature\'s shape')
    return dict(bg=float(wide.get("bg", 0.0)), sink=sink)


def _wide_forward(fb, wd, wfeat, opacity, op_fs):
    """the wide set over the batch's sorted lists, 32 channels at a time (splat_alpha_blending_forward_batch_set): [F, c, H, W].
    Every chunk leaves its own final_T / ncontrib (in ``wd``), packed records and cull words (pooled on the batch) for its
    backward: the row's fb.pack / final_T / ncontrib / cull_flags are not touched (the row's backward reads them), and a chunk's
    cull words are those of ITS forward kernel (a narrow chunk's hold the applied pairs, a wide one's the geometric cull's)."""
    lib, st = L.lib(), L.stream()
    F, P, W, H, cap = fb.F, fb.P, fb.W, fb.H, fb.capacity
    c = int(wfeat.shape[1])
    chunks = [(c0, min(32, c - c0)) for c0 in range(0, c, 32)]
    out = torch.empty(F, c, H, W, dtype=torch.float32, device=fb.dev)
    wd["chunks"] = chunks
    wd["final_T"] = torch.empty(len(chunks), F, H, W, dtype=torch.float32, device=fb.dev)
    wd["ncontrib"] = torch.empty(len(chunks), F, H, W, dtype=torch.int32, device=fb.dev)
    for k, (c0, cn) in enumerate(chunks):
        pack = fb._set_buffer(("wide", "pack", k), F * P * int(lib.splat_blend_pack_floats(cn)))
        cull = fb._set_buffer(("wide", "cull", k), F * cap)          # (raw 32-bit words)
        L.check(lib.splat_alpha_blending_forward_batch_set(
            F, P, c, c0, cn, L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(opacity), op_fs,
            L.ptr(wfeat), 0, L.ptr(fb.idx_sorted), L.ptr(fb.tile_range), cap, wd["bg"],
            W, H, L.ptr(out), L.ptr(wd["final_T"][k]), L.ptr(wd["ncontrib"][k]), L.ptr(pack), L.ptr(cull), st))
    return out


def _wide_backward(fb, wd, wfeat, opacity, op_fs, g, rec, d_feature):
    """per chunk of the wide set: the tile backward of its channel window from the records and cull words its forward left
    (splat_alpha_blending_backward_batch_set_packed) into ONE tail-record buffer (reused by the chunks), then
    splat_frames_wide_fold -- the tail records' ux uy ca cb cc into the SETS pair records ``rec`` the row's tile backward has written
    (not o: the opacity is detached), their feature part summed per Gaussian into ``d_feature`` [P, c] (None: not wanted)"""
    lib, st = L.lib(), L.stream()
    F, P, W, H, cap = fb.F, fb.P, fb.W, fb.H, fb.capacity
    c = int(wfeat.shape[1])
    g = L.need(g, "gradient of the wide output")
    if tuple(g.shape) != (F, c, H, W):
        raise ValueError(f"the gradient of the wide output must be [{F}, {c}, {H}, {W}]")
    from .gs.raster_ops import _debug_T_front
    tail = fb._set_buffer(("wide", "rec"), F * cap * int(lib.splat_blend_pair_stride(min(c, 32), 0, 0)))
    row_stride = int(lib.splat_blend_sets_pair_stride(fb.C))
    for k, (c0, cn) in enumerate(wd["chunks"]):
        pack = fb._set_buffer(("wide", "pack", k), F * P * int(lib.splat_blend_pack_floats(cn)))
        cull = fb._set_buffer(("wide", "cull", k), F * cap)
        L.check(lib.splat_alpha_blending_backward_batch_set_packed(
            F, P, c, c0, cn, L.ptr(fb.idx_sorted), L.ptr(fb.tile_range), cap,
            wd["bg"], W, H, L.ptr(wd["final_T"][k]), L.ptr(wd["ncontrib"][k]), L.ptr(g), L.ptr(fb.slot_sorted),
            L.ptr(tail), L.ptr(pack), L.ptr(cull), L.ptr(_debug_T_front(F * H, W, fb.dev)), st))
        L.check(lib.splat_frames_wide_fold(
            F, P, cn, cap, L.ptr(fb.goff), L.ptr(tail), L.ptr(rec), row_stride,
            L.ptr(d_feature), c, c0, st))


def _parse_sets(sets, F, P):
    """``sets`` -> (meta: per set (width | "depth", bg, detach_opacity, taps); parts: per set the (channels, per_frame) of every
    tensor its feature is made of -- () for the depth; the flat list of those tensors)"""
    meta, parts, feats = [], [], []
    for s_ in sets:
        f = s_["feature"]
        common = (float(s_.get("bg", 0.0)), bool(s_.get("detach_opacity", False)), bool(s_.get("taps", False)))
        if isinstance(f, str):
            if f != "depth":
                raise ValueError('a set\'s feature is a tensor, a list of tensors or the string "depth"')
            meta.append(("depth",) + common)
            parts.append(())
            continue
        pp = []
        for t in (list(f) if isinstance(f, (list, tuple)) else [f]):
            if not isinstance(t, Tensor) or t.dim() not in (2, 3):
                raise ValueError("a feature tensor is [P, c] (shared by the frames) or [F, P, c] (one row set per frame)")
            if t.dim() == 3 and (t.shape[0] != F or t.shape[1] != P):
                raise ValueError(f"a per-frame feature tensor must be [F={F}, P={P}, c], got {tuple(t.shape)}")
            if t.dim() == 2 and t.shape[0] != P:
                raise ValueError(f"a feature tensor must be [P={P}, c], got {tuple(t.shape)}")
            pp.append((int(t.shape[-1]), t.dim() == 3))
            feats.append(t)
        meta.append((sum(c for c, _ in pp),) + common)
        parts.append(tuple(pp))
    return tuple(meta), tuple(parts), feats


def _has_sources(parts) -> bool:
    """does any set consist of several tensors or of a per-frame tensor? (then the row is described by sources)"""
    return any(len(pp) > 1 or (len(pp) == 1 and pp[0][1]) for pp in parts)


def _source_tensor(t: Tensor, per_frame: bool, F: int, P: int) -> Tensor:
    """a source the kernels read in place: float32 on the device, dense rows; a per-frame tensor may be a strided view
    (frame stride >= P * c), anything else is made contiguous"""
    if not per_frame:
        return L.need(t, "feature")
    cn = t.shape[2]
    if t.is_cuda and t.dtype == torch.float32 and t.stride(2) == 1 and t.stride(1) == cn and t.stride(0) >= P * cn:
        L.need(t[0], "feature")      # (device gate; a frame's rows are contiguous)
        return t
    return L.need(t, "feature")


def _blend_sources_forward(fb, meta, parts, feats, opacity, K):
    """Forward compositing of a row described by SOURCES (splat_alpha_blending_forward_batch_sources): every tensor of every set
    is read in place -- shared rows [P, c], per-frame rows [F, P, c] (any frame stride), the per-frame depth."""
    lib, st = L.lib(), L.stream()
    F, P, W, H, C, cap = fb.F, fb.P, fb.W, fb.H, fb.C, fb.capacity
    widths = [1 if m[0] == "depth" else m[0] for m in meta]
    plan = _one_pass_plan(meta, widths, C)
    cache = fb.__dict__.setdefault("_bgc", {})
    bgc = cache.get(meta)
    if bgc is None:
        bgc = torch.tensor([bg for (w, bg, _, _), n in zip(meta, widths) for _ in range(n)], dtype=torch.float32, device=fb.dev)
        cache[meta] = bgc
    nsrc = sum(1 if w == "depth" else len(pp) for (w, _, _, _), pp in zip(meta, parts))    # the depth counts as a source
    if nsrc > L.MAX_SOURCES:
        raise ValueError(f"at most {L.MAX_SOURCES} feature sources per row (the depth counts as one), got {nsrc}")
    table = (L.FeatureSource * L.MAX_SOURCES)()
    n, c0, it = 0, 0, iter(feats)
    for (w, _, _, _), pp in zip(meta, parts):
        if w == "depth":
            table[n].c0, table[n].cn, table[n].feature, table[n].frame_stride = c0, 1, fb.depth.data_ptr(), P
            n += 1
            c0 += 1
            continue
        for cn, per_frame in pp:
            t = next(it)
            table[n].c0, table[n].cn, table[n].feature = c0, cn, t.data_ptr()
            table[n].frame_stride = int(t.stride(0)) if per_frame else 0
            n += 1
            c0 += cn
    out = torch.empty(F, C, H, W, dtype=torch.float32, device=fb.dev)
    gs_idx = torch.empty(F, H, W, K, dtype=torch.int32, device=fb.dev) if K > 0 else None
    L.check(lib.splat_alpha_blending_forward_batch_sources(
        F, P, C, n, table, L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(opacity), 0,
        L.ptr(fb.idx_sorted), L.ptr(fb.tile_range), cap, L.ptr(bgc), W, H, K, 0,
        L.ptr(out), L.ptr(fb.final_T), L.ptr(fb.ncontrib), L.ptr(gs_idx), L.ptr(fb.pack), L.ptr(fb.cull_flags), st))
    # (the forward-pack decision is taken HERE and kept in the autograd context: an option flipped between this forward and its
    #  backward must not change what the backward stages)
    return out, gs_idx, dict(plan=plan, tens=None, row=None, widths=widths, std=_uses_forward_pack(plan, C), out_row=out)


def _blend_sets_forward(fb, meta, feats, opacity, op_fs, K):
    """Forward compositing of the sets' row for all frames.  When the sets fit the one-pass backward every set is read from its
    own tensor (shared features [P,c], the per-frame depth [F,P,1]) -- no [F,P,C] row is materialised; otherwise the row is
    concatenated and the per-set passes use it.  Returns (out [F,C,H,W], gs_idx, state for _blend_sets_backward)."""
    lib, st = L.lib(), L.stream()
    F, P, W, H, C, cap = fb.F, fb.P, fb.W, fb.H, fb.C, fb.capacity
    widths = [1 if m[0] == "depth" else m[0] for m in meta]
    one_pass_wanted = OPTIONS["sets_one_pass"]
    plan = _one_pass_plan(meta, widths, C) if one_pass_wanted else None
    if plan is None and one_pass_wanted and not fb.__dict__.get("_warned_per_set"):
        fb.__dict__["_warned_per_set"] = True   # (once per batch object)
        warnings.warn("FrameBatch.render_sets: these feature sets do not fit the one-pass backward (one set per routing group -- "
                      "taps / live opacity / detached opacity -- of at most 4 / 4 / 20 channels): the backward runs one pass of "
                      "the tile kernels per set", RuntimeWarning, stacklevel=3)
    tens, it = [], iter(feats)
    for w, _, _, _ in meta:
        tens.append(fb.depth if w == "depth" else _points(next(it), "feature", w))
    cache = fb.__dict__.setdefault("_bgc", {})
    bgc = cache.get(meta)
    if bgc is None:
        bgc = torch.tensor([bg for (w, bg, _, _), n in zip(meta, widths) for _ in range(n)], dtype=torch.float32, device=fb.dev)
        cache[meta] = bgc
    out = torch.empty(F, C, H, W, dtype=torch.float32, device=fb.dev)
    gs_idx = torch.empty(F, H, W, K, dtype=torch.int32, device=fb.dev) if K > 0 else None
    row = None
    if plan is None:
        row = torch.cat([t if m[0] == "depth" else t.unsqueeze(0).expand(F, P, t.shape[1]) for t, m in zip(tens, meta)],
                        dim=2).contiguous()
        L.check(lib.splat_alpha_blending_forward_batch(
            F, P, C, L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(opacity), op_fs, L.ptr(row),
            P * C, L.ptr(fb.idx_sorted), L.ptr(fb.tile_range), cap, 0.0, L.ptr(bgc),
            W, H, K, 0, L.ptr(out), L.ptr(fb.final_T), L.ptr(fb.ncontrib), L.ptr(gs_idx),
            L.ptr(fb.pack), L.ptr(fb.cull_flags), st))
    else:
        tabs = _set_tables(meta, plan, tens, P)
        L.check(lib.splat_alpha_blending_forward_batch_sets(
            F, P, C, tabs["c0"], tabs["cn"], tabs["feat"], tabs["fs"], L.ptr(fb.uv), L.ptr(fb.conic),
            L.ptr(opacity), op_fs, L.ptr(fb.idx_sorted), L.ptr(fb.tile_range), cap, L.ptr(bgc),
            W, H, K, 0, L.ptr(out), L.ptr(fb.final_T), L.ptr(fb.ncontrib), L.ptr(gs_idx),
            L.ptr(fb.pack), L.ptr(fb.cull_flags), st))
    return out, gs_idx, dict(plan=plan, tens=tens, row=row, widths=widths, std=_uses_forward_pack(plan, C), out_row=out)


def _set_tables(meta, plan, tens, P):
    """ctypes tables (three routing groups) of a one-pass plan: first row channel, width, feature pointer, frame stride"""
    c0s, cns, bgs, _, _ = plan
    groups = _set_groups(meta)
    ptr, fs = [0, 0, 0], [0, 0, 0]
    for (w, _, _, _), t, g in zip(meta, tens or [None] * len(meta), groups):
        ptr[g] = 0 if t is None else t.data_ptr()   # (None: a row by sources -- its backward stages the forward's records)
        fs[g] = P if w == "depth" else 0        # the depth [F,P,1] is per frame, feature rows are shared
    i3, f3 = ctypes.c_int32 * 3, ctypes.c_float * 3
    return dict(c0=i3(*c0s), cn=i3(*cns), bg=f3(*bgs), feat=(ctypes.c_void_p * 3)(*ptr), fs=(ctypes.c_int64 * 3)(*fs))


def _blend_sets_backward_one_pass(fb, meta, state, grads, opacity, op_fs, want_abs):
    """ONE pass of the tile kernels for the three sets (splat_alpha_blending_backward_batch_sets): every set's image gradient
    from its own tensor.  Returns the pair-record buffer.  With ``fb.fuse_l1(...)`` armed the incoming gradient tensors are
    placeholders: the kernel derives the L1 loss' gradient from the forward's output row and the target images."""
    lib, st = L.lib(), L.stream()
    F, P, W, H, C, cap = fb.F, fb.P, fb.W, fb.H, fb.C, fb.capacity
    plan, tens = state["plan"], state["tens"]
    tabs = _set_tables(meta, plan, tens, P)
    groups = _set_groups(meta)
    dl = [0, 0, 0]
    keep = []
    l1 = fb.__dict__.pop("_l1", None)
    if l1 is not None:
        from .gs.raster_ops import _debug_T_front
        row = state.get("out_row")
        if row is None or tuple(row.shape) != (F, C, H, W) or not L.get_option("bwd_quarters"):
            raise ValueError("the loss-fused backward needs the forward's output row and the quarter-list kernels")
        scale = [0.0, 0.0, 0.0]
        for tgt, wgt, w, grp in zip(l1["targets"], l1["weights"], state["widths"], groups):
            t = L.need(tgt, "target image")
            if tuple(t.shape) != (F, w, H, W):
                raise ValueError(f"a set's target image must be [F={F}, {w}, H, W]")
            keep.append(t)
            dl[grp] = t.data_ptr()
            scale[grp] = float(wgt) / (F * w * H * W)          # d (weight * mean |pred - target|) / d pred
        sums = L.need(l1["sums"], "l1 sums")
        if sums.numel() != 3 * F * fb.T:
            raise ValueError(f"l1 sums must be [F={F}, tiles={fb.T}, 3]")
        rec = fb._set_buffer(("rec", "sets"), F * cap * int(lib.splat_blend_sets_pair_stride(C)))
        std = state["std"] if "std" in state else _uses_forward_pack(plan, C)
        pack = None if std else fb._set_buffer(("pack", "sets"), F * P * int(lib.splat_blend_sets_pack_floats()))
        L.check(lib.splat_alpha_blending_backward_batch_sets_l1(
            F, P, C, tabs["c0"], tabs["cn"], tabs["bg"], L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(opacity),
            op_fs, tabs["feat"], tabs["fs"], L.ptr(fb.idx_sorted), L.ptr(fb.tile_range), cap,
            W, H, L.ptr(fb.final_T), L.ptr(fb.ncontrib), L.ptr(row), (ctypes.c_void_p * 3)(*dl),
            (ctypes.c_float * 3)(*scale), L.ptr(sums), want_abs, L.ptr(fb.slot_sorted), L.ptr(rec), L.ptr(pack),
            L.ptr(fb.cull_flags), L.ptr(_debug_T_front(F * H, W, fb.dev)), L.ptr(fb.pack if (std or tens is None) else None), st))
        # the slab order of the three groups: (tap set, second set, detached set) -> set index of the caller's list
        l1["group_of_set"] = list(groups)
        return rec
    for g_, w, grp in zip(grads, state["widths"], groups):
        t = L.need(g_, "dL_dout") if g_ is not None else torch.zeros(F, w, H, W, dtype=torch.float32, device=fb.dev)
        if tuple(t.shape) != (F, w, H, W):
            raise ValueError("image gradient of a set must be [F, c, H, W]")
        keep.append(t)
        dl[grp] = t.data_ptr()
    from .gs.raster_ops import _debug_T_front
    rec = fb._set_buffer(("rec", "sets"), F * cap * int(lib.splat_blend_sets_pair_stride(C)))
    # the renderer's own plan (rgb 0-2 with the taps | depth 3 | 19 detached attributes 4-22): the tile kernel stages the records
    # the FORWARD packed (fb.pack) -- no packing launch, no second record array; other plans pack their own (a row described by
    # sources -- tens is None -- out of the forward's records, which hold the row's channels)
    std = state["std"] if "std" in state else _uses_forward_pack(plan, C)     # decided at forward time
    pack = None if std else fb._set_buffer(("pack", "sets"), F * P * int(lib.splat_blend_sets_pack_floats()))
    L.check(lib.splat_alpha_blending_backward_batch_sets_packed(
        F, P, C, tabs["c0"], tabs["cn"], tabs["bg"], L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(opacity),
        op_fs, L.ptr(None), 0, tabs["feat"], tabs["fs"], L.ptr(fb.idx_sorted),
        L.ptr(fb.tile_range), cap, W, H, L.ptr(fb.final_T), L.ptr(fb.ncontrib), L.ptr(None),
        (ctypes.c_void_p * 3)(*dl), want_abs, L.ptr(fb.slot_sorted), L.ptr(rec), L.ptr(pack), L.ptr(fb.cull_flags),
        L.ptr(_debug_T_front(F * H, W, fb.dev)), L.ptr(fb.pack if (std or tens is None) else None), st))
    return rec


def _uses_forward_pack(plan, C) -> bool:
    """does the one-pass backward of this plan stage the records the FORWARD packed (no packing launch, no pack scratch)?  The C
    library owns the condition (splat_blend_sets_uses_forward_pack: the renderer's own plan with the cull words)."""
    from .gs.raster_ops import OPTIONS as RO
    if plan is None or not RO["sets_fwdrec"]:
        return False
    i3 = ctypes.c_int32 * 3
    return bool(L.lib().splat_blend_sets_uses_forward_pack(C, i3(*plan[0]), i3(*plan[1]), 1))


def _check_set_features(meta, feats, P):
    """every shared feature tensor of the sets is [P, c] with the width its set declares (the kernels index rows 0 .. P-1)"""
    it = iter(feats)
    for w, _, _, _ in meta:
        if w == "depth":
            continue
        t = next(it)
        if t.dim() != 2 or t.shape[0] != P or t.shape[1] != w:
            raise ValueError(f"a set's feature must be [P={P}, {w}], got {tuple(t.shape)}")


def _set_groups(meta):
    """Routing group of every set: 0 = feeds the taps, 1 = live opacity without taps, 2 = opacity.detach()."""
    return [0 if taps else (2 if detach else 1) for (_, _, detach, taps) in meta]


def _one_pass_plan(meta, widths, C):
    """Can ONE pass of splat_alpha_blending_backward_batch_sets serve these sets?  At most one set per routing group, the
    tap set blended with the live opacity, widths <= (4, 4, 20), C <= 28.  Returns (c0[3], cn[3], bg[3], depth row channel
    or -1, index of the tap set or None), or None: the per-set passes run."""
    if C > 28:
        return None
    groups = _set_groups(meta)
    if len(set(groups)) != len(groups):
        return None
    c0s, cns, bgs, depth_ch, tap_set = [0, 0, 0], [0, 0, 0], [0.0, 0.0, 0.0], -1, None
    c0 = 0
    for si, ((w, bg, detach, taps), cn, g) in enumerate(zip(meta, widths, groups)):
        if (taps and detach) or cn > (4, 4, 20)[g]:
            return None
        c0s[g], cns[g], bgs[g] = c0, cn, bg
        if w == "depth":
            depth_ch = c0
        if taps:
            tap_set = si
        c0 += cn
    return c0s, cns, bgs, depth_ch, tap_set


def _static_geometry(fb, xyz, scales, uquats, opacity, offsets, extr, intr):
    """the static geometry of ``render`` / ``render_sets`` normalised and checked against the batch: (xyz, scales, uquats, opacity,
    offsets [F, P, 3] or None, the batch's ``_Camera``); the opacity's size is the caller's check"""
    xyz = _points(xyz, "xyz", 3)
    scales = _points(scales, "scales", 3)
    uquats = _points(uquats, "uquats", 4)
    opacity = L.need(opacity, "opacity")
    P, F = fb.P, fb.F
    cam = _Camera(extr, intr, F)
    if xyz.shape[0] != P or scales.shape[0] != P or uquats.shape[0] != P:
        raise ValueError(f"the batch was built for {P} Gaussians")
    off = L.need(offsets, "offsets") if offsets is not None else None
    if off is not None and tuple(off.shape) != (F, P, 3):
        raise ValueError(f"offsets must be [F={F}, P={P}, 3]")
    if off is None and F > 1 and cam.extr_fs == 0:
        raise ValueError("several frames of static Gaussians need per-frame offsets or per-frame cameras")
    return xyz, scales, uquats, opacity, off, cam


class _RenderSets(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, scales, uquats, opacity, offsets, extr, fb, meta, K, nearest, extent, sink, intr, wd, *feats):
        wfeat = None
        if wd is not None:        # the wide set's feature rides last
            feats, wfeat = feats[:-1], L.need(feats[-1], "wide feature")
        xyz, scales, uquats, opacity, off, cam = _static_geometry(fb, xyz, scales, uquats, opacity, offsets, extr, intr)
        if opacity.numel() != fb.P:
            # (the Gaussian-side backward sums the opacity gradient over the frames: a per-frame opacity [F,P,1] has no entry point)
            raise ValueError(f"opacity must hold one value per Gaussian ({fb.P}), shared by the frames; got {tuple(opacity.shape)}")
        _check_set_features(meta, feats, fb.P)
        ctx.gen = fb._begin_forward()
        fb._geometry(xyz, scales, uquats, off, cam, nearest, extent, opacity)
        op_fs = 0
        out, gs_idx, ctx.blend = _blend_sets_forward(fb, meta, feats, opacity, op_fs, K)
        if wd is not None and ctx.blend["plan"] is None:
            raise ValueError("render_sets(wide=...) needs sets that fit the one-pass backward")
        ctx.fb, ctx.meta, ctx.sink, ctx.K = fb, meta, sink, K
        ctx.cam, ctx.off = cam, off
        ctx.cam_versions = _versions(cam.extr, cam.intr, off)
        ctx.wd = wd
        wide_out = ()
        if wd is not None:
            wide_out = (_wide_forward(fb, wd, wfeat, opacity, op_fs),)
            feats = tuple(feats) + (wfeat,)
        ctx.save_for_backward(xyz, scales, uquats, opacity, *feats)
        ctx.set_materialize_grads(False)
        if gs_idx is not None:
            ctx.mark_non_differentiable(gs_idx)
        return tuple(_split_row(out, meta)) + wide_out + (gs_idx,)

    LEAVES = ("xyz", "scales", "uquats", "opacity")
    ARGS = _args_of(forward, *LEAVES)
    FEATS = ARGS.index("feats")
    PAD = (None,) * (FEATS - len(LEAVES))

    @staticmethod
    def backward(ctx, *grads):
        A, fb = _RenderSets, ctx.fb
        fb._check_generation(ctx.gen)
        xyz, scales, uquats, opacity = ctx.saved_tensors[:4]
        feats = ctx.saved_tensors[4:]
        wd, wfeat, g_wide = ctx.wd, None, None
        if wd is not None:
            feats, wfeat = feats[:-1], feats[-1]
            g_wide = grads[len(ctx.meta)]
        _check_versions(ctx.cam_versions, "a camera / offset tensor")
        camc = ctx.cam.struct(ctx.off)
        meta, sink = ctx.meta, (ctx.sink or {})
        lib, st = L.lib(), L.stream()
        F, P, W, H, C, cap = fb.F, fb.P, fb.W, fb.H, fb.C, fb.capacity
        dev = fb.dev
        widths = ctx.blend["widths"]
        like = {"xyz": xyz, "scales": scales, "uquats": uquats, "opacity": opacity}
        bufs = {k: (sink[k] if k in sink else torch.zeros_like(v)) for k, v in like.items()}   # every set accumulates
        ret = tuple(None if k in sink else bufs[k] for k in A.LEAVES)
        wanted = ctx.needs_input_grad[A.FEATS:]               # per feature tensor: the sets' tensors, then the wide set's
        op_fs = 0
        from .gs.raster_ops import _debug_T_front
        plan = ctx.blend["plan"]
        if plan is not None:
            # the sets share the alpha / transmittance replay: ONE pass of the tile kernels and ONE Gaussian-side reduction
            # route dL/dalpha of every set where the reference's three autograd nodes would
            depth_ch, has_tap = plan[3], plan[4] is not None
            want_abs = 1 if (has_tap and fb.want_abs) else 0
            dfe, features = _group_grads(meta, plan, feats, grads, wanted)
            rec = _blend_sets_backward_one_pass(fb, meta, ctx.blend, grads[:len(meta)], opacity, op_fs, want_abs)
            # the wide set's chunks: their geometry terms into the pair records, their feature sums into the feature's gradient
            d_wide = () if wd is None else (None,) if g_wide is None else _side_backward(
                wanted[len(feats)], wd["sink"], wfeat, lambda buf: _wide_backward(fb, wd, wfeat, opacity, op_fs, g_wide, rec, buf))
            L.check(lib.splat_frames_gauss_backward_static_sets_cam(
                F, P, C, W, H, cap, L.ptr(rec), L.ptr(fb.goff), L.ptr(fb.radius),
                L.ptr(xyz), L.ptr(scales), L.ptr(uquats), ctypes.byref(camc), 1, L.ptr(bufs["xyz"]), L.ptr(bufs["scales"]),
                L.ptr(bufs["uquats"]), L.ptr(bufs["opacity"]), *features, depth_ch,
                L.ptr(fb.tap if has_tap else None), L.ptr(fb.abs_tap if (has_tap and want_abs) else None),
                L.ptr(fb.radii_max if has_tap else None), st))
            return ret + A.PAD + dfe + d_wide
        row, dfe = ctx.blend["row"], []
        dL = torch.cat([(g if g is not None else torch.zeros(F, w, H, W, dtype=torch.float32, device=dev))
                        for g, w in zip(grads[:len(meta)], widths)], dim=1).contiguous()
        c0, fi = 0, 0
        for si, ((w, bg, detach, taps), g) in enumerate(zip(meta, grads[:len(meta)])):
            cn = widths[si]
            is_depth = w == "depth"
            dfeat = None
            if not is_depth:
                dfeat = torch.zeros_like(feats[fi]) if g is not None and wanted[fi] else None
                dfe.append(dfeat)
                fi += 1
            if g is not None:
                want_abs = 1 if (taps and fb.want_abs) else 0
                ncp = int(lib.splat_blend_pair_stride(cn, want_abs, 0))
                rec = fb._set_buffer(("rec", si), F * cap * ncp)
                pack = fb._set_buffer(("pack", si), F * P * int(lib.splat_blend_pack_floats(cn)))
                L.check(lib.splat_alpha_blending_backward_batch_set(
                    F, P, C, c0, cn, L.ptr(fb.uv), L.ptr(fb.conic), L.ptr(opacity),
                    op_fs, L.ptr(row), P * C, L.ptr(fb.idx_sorted), L.ptr(fb.tile_range),
                    cap, bg, W, H, L.ptr(fb.final_T), L.ptr(fb.ncontrib), L.ptr(dL),
                    want_abs, L.ptr(fb.slot_sorted), L.ptr(rec), L.ptr(pack), L.ptr(_debug_T_front(F * H, W, dev)), st))
                L.check(lib.splat_frames_gauss_backward_static_cam(
                    F, P, cn, W, H, cap, want_abs, L.ptr(rec), L.ptr(fb.goff),
                    L.ptr(fb.radius), L.ptr(xyz), L.ptr(scales), L.ptr(uquats), ctypes.byref(camc), 1, L.ptr(bufs["xyz"]),
                    L.ptr(bufs["scales"]), L.ptr(bufs["uquats"]), L.ptr(bufs["opacity"]), L.ptr(dfeat), cn,
                    1 if detach else 0, 0 if is_depth else -1, L.ptr(fb.tap if taps else None),
                    L.ptr(fb.abs_tap if (taps and want_abs) else None), L.ptr(fb.radii_max if taps else None), st))
            c0 += cn
        return ret + A.PAD + tuple(dfe) + (() if wd is None else (None,))


class _RenderFrames(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, scales, uquats, opacity, feature, offsets, extr, fb: FrameBatch, bg, nearest, extent, sink, intr=None):
        xyz, scales, uquats, opacity, off, cam = _static_geometry(fb, xyz, scales, uquats, opacity, offsets, extr, intr)
        feature = _points(feature, "feature", fb.C)
        if opacity.numel() != fb.P or feature.shape[0] != fb.P:
            raise ValueError(f"the batch was built for {fb.P} Gaussians")
        ctx.gen = fb._begin_forward()
        out = fb._forward_onecall(xyz, scales, uquats, opacity, feature, off, cam, bg, nearest, extent)
        ctx.fb, ctx.bg, ctx.sink = fb, bg, sink
        ctx.cam, ctx.off = cam, off
        ctx.cam_versions = _versions(cam.extr, cam.intr, off)
        ctx.save_for_backward(xyz, scales, uquats, opacity, feature)
        return out

    LEAVES = ("xyz", "scales", "uquats", "opacity", "feature")
    ARGS = _args_of(forward, *LEAVES)
    PAD = (None,) * (len(ARGS) - len(LEAVES))

    @staticmethod
    def backward(ctx, dL_dout):
        A, fb = _RenderFrames, ctx.fb
        fb._check_generation(ctx.gen)
        xyz, scales, uquats, opacity, feature = ctx.saved_tensors
        _check_versions(ctx.cam_versions, "a camera / offset tensor")
        g = L.need(dL_dout, "dL_dout")
        sink = ctx.sink or {}
        like = {"xyz": xyz, "scales": scales, "uquats": uquats, "opacity": opacity, "feature": feature}
        # one accumulate flag for the launch: with a sink in play the buffers autograd receives start from zero
        fresh = torch.zeros_like if sink else torch.empty_like
        bufs = {k: (sink[k] if k in sink else fresh(v)) for k, v in like.items()}
        from .gs.raster_ops import _debug_T_front
        dbg = _debug_T_front(fb.F * fb.H, fb.W, g.device)
        fb._backward_onecall(g, xyz, scales, uquats, ctx.off, ctx.cam, ctx.bg, bufs, accumulate=bool(sink), dbg=dbg)
        fb._pending = False        # (frame_rasterization's pool: the batch's forward has had its backward)
        return tuple(None if k in sink else bufs[k] for k in A.LEAVES) + A.PAD


# ------------------------------------------------------------------ ONE frame behind one call per direction
# gs.rasterization's chain -- project_point -> compute_cov3d -> ewa_project -> sort_gaussian -> alpha_blending (reference:
# src/submodules/dptr/dptr/gs/__init__.py:28-100) -- for a caller that wants the image of ONE frame: a FrameBatch of one frame
# does it with the launches of splat_frames_forward / _backward (fused preprocess, binning with reach masks, sort, compositing |
# tile backward, Gaussian-side backward with the projection chain), one autograd node, a dozen tensor allocations less than the
# operator chain.  The forward reads the frame's pair count between binning and sort (frame_rasterization's docstring: the ONE
# host synchronisation sort_gaussian makes in the chain, so that a frame never loses pairs to buffers an earlier call sized), which
# is why it enqueues its four steps itself; inside a stream capture it is the one crossing of the C ABI, and the backward always
# is.  The batches are pooled by shape: a batch whose forward still waits for its backward is not
# reused (two views rendered before one backward get two batches; at most POOL_MAX per shape, then the oldest is reused and ITS
# late backward raises).  Over all shapes the pool holds at most POOL_TOTAL batches: a trainer that densifies renders a new P every
# interval, and each batch owns keys, pair records, cull flags and bin scratch.  Beyond the total the least recently used shape
# gives up its oldest batch -- the pool only drops its reference: a batch whose backward is pending lives on through its autograd
# node and is freed with it.
_FRAME_POOL: Dict[tuple, list] = {}     # shape -> its batches; the dict's order is the order of last use
POOL_MAX = 4
POOL_TOTAL = 8


def clear_frame_pool() -> None:
    """drop every pooled batch of ``frame_rasterization`` (their device memory goes back to the allocator once no pending
    backward holds them); the next call builds a new batch"""
    _FRAME_POOL.clear()
    frame_rasterization.last = None


def _pooled_batch(P: int, W: int, H: int, C: int, dev, needs_grad: bool) -> FrameBatch:
    key = (str(dev), int(P), int(W), int(H), int(C))
    pool = _FRAME_POOL.pop(key, [])
    _FRAME_POOL[key] = pool                 # (most recently used: last)
    fb = next((b for b in pool if not getattr(b, "_pending", False)), None)
    if fb is None:
        if len(pool) >= POOL_MAX:
            fb = pool.pop(0)
        else:
            while sum(len(v) for v in _FRAME_POOL.values()) >= POOL_TOTAL:
                lru = next(iter(_FRAME_POOL))
                _FRAME_POOL[lru].pop(0)
                if not _FRAME_POOL[lru]:
                    del _FRAME_POOL[lru]
            fb = FrameBatch(1, P, W, H, C, dev)
            fb._measured = True             # sized per call from the frame's own pair count (_forward_onecall)
        pool.append(fb)
    fb._pending = bool(needs_grad)
    return fb


def frame_rasterization(xyz: Tensor, scale: Tensor, rotate: Tensor, opacity: Tensor, feature: Tensor, extr: Tensor, W: int, H: int,
                        bg: float = 0.0, intr: Optional[Tensor] = None, offset: Optional[Tensor] = None, nearest: float = 0.01,
                        extent: float = 1.3, grad_sink: Optional[Dict[str, Tensor]] = None) -> Tensor:
    """image [C, H, W] of one frame: the orthographic camera ``extr`` -- or, with ``intr`` (fx, fy, cx, cy), the pinhole camera
    of ``gs.rasterization`` -- over ``xyz (+ offset)``; differentiable w.r.t. xyz, scale, rotate, opacity, feature (cameras are
    not differentiated).  ``grad_sink`` as in ``FrameBatch.render`` (names xyz, scales, uquats, opacity, feature).  The batch that
    rendered the frame is ``frame_rasterization.last`` (its ``tap`` / ``radii_max`` after the backward: the densification taps).

    Pair capacity: the caller has no capacity knob, so no call returns an image with dropped pairs.  Every call reads the
    frame's pair count between binning and sort -- ONE host synchronisation, the one ``gs.sort_gaussian`` makes in the operator
    chain -- and grows the pooled batch's pair buffers (count * 1.25 + 1024) when another camera, a zoom or grown scales hold
    more pairs than the buffers were sized for.  A batch whose backward is pending is not taken from the pool (also not by a
    call under ``no_grad``), so a resize never touches lists a backward still reads; past ``POOL_MAX`` live forwards of one shape
    the oldest batch is reused and its late backward raises before it reads anything.  INSIDE a stream capture (``torch.cuda.graph``) nothing is synchronised or
    resized: the capacity is whatever the warm-up calls reserved, the whole forward is one ``splat_frames_forward``, and a
    frame that outgrows the capacity at a replay drops its surplus pairs -- ``frame_rasterization.last.check()`` after the
    replay raises then, as for an explicit ``FrameBatch``."""
    P, C = feature.shape
    needs = torch.is_grad_enabled() and any(t.requires_grad for t in (xyz, scale, rotate, opacity, feature))
    fb = _pooled_batch(P, W, H, C, xyz.device, needs)
    off = None if offset is None else offset.reshape(1, P, 3)
    out = fb.render(xyz, scale, rotate, opacity, feature, off, extr, bg=bg, nearest=nearest, extent=extent, grad_sink=grad_sink,
                    intr=intr)
    frame_rasterization.last = fb
    return out[0]

