"""2-D track targets of the trainer's optical-flow term (src/trainer_fragGS.py:528-569), packed for ``losses.track_loss``.

Per frame pair (ids1, ids2) the reference reads two TAPIR files through ``load_target_tracks``: the query points of frame ids1
(``{ids1}_{ids1}.npy[:, :2]``, pixel xy) and their tracks in frame ids2 (``{ids1}_{ids2}.npy``: x, y, occlusion logit,
expected-distance logit).  It marks the truncated query pixels in a mask and gathers the prediction with ``pred[mask]`` -- in
RASTER order -- next to the target rows in FILE order: the i-th masked pixel in raster order is compared with target row i.
This pairing is by rank, not by query index; the two agree only when the file lists its queries in raster order (TAPIR's query
grids do).  ``TrackTargets`` keeps exactly that pairing: the pixel indices sorted, the target rows as given.  The reference
needs unique query pixels (its boolean indexing fails on a shape mismatch otherwise); here a duplicate is a ``ValueError``.

A batch of F pairs is one ``TrackTargets`` in CSR form: ``offsets`` [F + 1] (int64), ``pixels`` [Q] (int32, y * W + x,
strictly ascending within a frame), ``targets`` [Q, 4] (float32).  The per-frame counts stay on the host, so ``cat`` builds a
batch without a host synchronisation.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch
from torch import Tensor


def _as_cpu(a, dtype) -> Tensor:
    t = a if isinstance(a, Tensor) else torch.as_tensor(np.asarray(a))
    return t.detach().to("cpu", dtype)


def _upload(t: Tensor, device) -> Tensor:
    """a host tensor to ``device`` without waiting for the stream (pinned staging buffer, asynchronous copy)"""
    device = torch.device(device)
    if device.type == "cuda" and t.device.type == "cpu":
        return t.pin_memory().to(device, non_blocking=True)
    return t.to(device)


class TrackTargets:
    """query pixels and target rows of F frame pairs (CSR); ``counts[f]`` = the number of queries of frame f (host ints)"""

    def __init__(self, offsets: Tensor, pixels: Tensor, targets: Tensor, H: int, W: int, counts: Sequence[int]):
        self.offsets, self.pixels, self.targets = offsets, pixels, targets
        self.H, self.W = int(H), int(W)
        self.counts: Tuple[int, ...] = tuple(int(c) for c in counts)
        if offsets.dtype != torch.int64 or pixels.dtype != torch.int32 or targets.dtype != torch.float32:
            raise ValueError("TrackTargets: offsets int64, pixels int32, targets float32")
        if tuple(offsets.shape) != (len(self.counts) + 1,) or pixels.shape != (sum(self.counts),) or \
                tuple(targets.shape) != (sum(self.counts), 4):
            raise ValueError("TrackTargets: offsets [F + 1], pixels [Q], targets [Q, 4] with Q = sum(counts)")

    @property
    def F(self) -> int:
        return len(self.counts)

    @property
    def Q(self) -> int:
        return int(self.pixels.shape[0])

    @property
    def device(self) -> torch.device:
        return self.pixels.device

    @classmethod
    def from_reference(cls, query_xy, target, H: int, W: int) -> "TrackTargets":
        """one frame pair from the arrays ``load_target_tracks`` returns: ``query_xy`` [Q, 2] (pixel xy of the queries in frame
        ids1) and ``target`` [Q, 4] (or [1, Q, 4]: x, y, occlusion logit, expected-distance logit in frame ids2).  The query
        coordinates are truncated toward zero (``.to(torch.int64)``), must lie inside the H x W image and be unique
        (``ValueError`` otherwise); the pixel indices are sorted, the target rows stay in file order."""
        H, W = int(H), int(W)
        q = _as_cpu(query_xy, torch.float32)
        t = _as_cpu(target, torch.float32)
        if q.dim() != 2 or q.shape[1] != 2:
            raise ValueError(f"query_xy must be [Q, 2], got {tuple(q.shape)}")
        Q = q.shape[0]
        if t.shape[-1] != 4 or t.numel() != 4 * Q:
            raise ValueError(f"target must be [Q, 4] (or [1, Q, 4]) with Q = {Q}, got {tuple(t.shape)}")
        if not bool(torch.isfinite(q).all()):
            raise ValueError("query_xy holds a non-finite coordinate")
        qi = q.to(torch.int64)
        px, py = qi[:, 0], qi[:, 1]
        if Q and not bool(((px >= 0) & (px < W) & (py >= 0) & (py < H)).all()):
            raise ValueError(f"a query pixel lies outside the {W} x {H} image")
        pix = py * W + px
        pix_sorted = torch.sort(pix).values
        if Q > 1 and bool((pix_sorted[1:] == pix_sorted[:-1]).any()):
            raise ValueError("query pixels must be unique (the reference's mask gather needs one query per pixel)")
        return cls(torch.tensor([0, Q], dtype=torch.int64), pix_sorted.to(torch.int32), t.reshape(Q, 4).contiguous(), H, W, [Q])

    def to(self, device) -> "TrackTargets":
        return TrackTargets(_upload(self.offsets, device), _upload(self.pixels, device), _upload(self.targets, device),
                            self.H, self.W, self.counts)

    @staticmethod
    def cat(parts: Sequence["TrackTargets"]) -> "TrackTargets":
        """the frame pairs of ``parts`` in order, one batch (the tensors are concatenated where they live; the offsets come from
        the host counts)"""
        parts = list(parts)
        if not parts:
            raise ValueError("TrackTargets.cat needs at least one part")
        H, W, dev = parts[0].H, parts[0].W, parts[0].device
        if any((p.H, p.W) != (H, W) or p.device != dev for p in parts):
            raise ValueError("TrackTargets.cat: every part must have the same image size and device")
        counts = [c for p in parts for c in p.counts]
        offsets = _upload(torch.tensor(np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]), dtype=torch.int64), dev)
        return TrackTargets(offsets, torch.cat([p.pixels for p in parts]), torch.cat([p.targets for p in parts]), H, W, counts)


def frame_weights(times1: Sequence[float], times2: Sequence[float], num_frames: int) -> Tensor:
    """the reference's frame-distance weights ``exp(-2 * |ids2 - ids1| / num_imgs)`` (src/trainer_fragGS.py:529-530) in float32,
    one per pair (a CPU tensor)"""
    t1 = torch.as_tensor(np.asarray(times1, dtype=np.float64))
    t2 = torch.as_tensor(np.asarray(times2, dtype=np.float64))
    if t1.shape != t2.shape or t1.dim() != 1:
        raise ValueError("times1 and times2 must be sequences of the same length")
    intervals = torch.abs(t2 - t1).float()
    return torch.exp(-2 * intervals / int(num_frames))
