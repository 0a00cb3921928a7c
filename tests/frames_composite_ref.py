"""The frame batch's compositing entry points (csrc/blend.hip: splat_alpha_blending_forward_batch* / _backward_batch*) against
the float64 reference of tests/composite_ref.py (test helper, no test functions; no GPU call at import).

Clips: F frames of ONE Gaussian count at one image size, every frame a decision-clear composite_ref.Scene with a name of its
own (the session caches of composite_ref are keyed by the name).
  opaque_x4   f0 = opaque_100x60; f1 = every radius 0 (an empty frame in mid-batch); f2 = f0 mirrored in u (u' = W - u, B' = -B)
              with opacity x 0.8 in float32 -- the clip's opacity is per frame, [F,P]; f3 = f0 with depth' = max + min - depth
              (the wall goes to the back)
  hard_x2     f0 = hard_64x48; f1 = the same operands with the reversed depth (one opacity array shared by the frames)
A derived frame starts from f0's radii after culling and pruning, recounts the tile rectangles for the moved centres and is
pruned to a fixed point like composite_ref._finish does it.

Driver: thin ctypes callers over splatter_a_video_amd._lib.  Every buffer a kernel writes is pre-filled with NaN or -1 (keys,
idx_sorted, slot_sorted, the pair records, the packed records, the cull words, the images), `capacity` is the fullest frame's
pairs + 37, so a slot no pair owns shows when something reads it.  The pair records of frame f are reduced per Gaussian with
splat_pair_records_segment_sum at f * capacity * stride and goff_incl[f] (reduce_frames; ``shift`` moves the read by whole
slots: the CPU tests show that the bars notice a shift of one) and sliced by gauss_backward_ref.plain_layout / sets_layout.

Reference: composite_ref.walk / forward / backward per frame, cached per session; the comparison rules are those of
tests/test_gpu_composite_reference.py (integers exact, values within K x companion, K from
profiles/composite_reference_cpu_float32.json)."""
from __future__ import annotations

import ctypes
import dataclasses
import json
import os

import numpy as np

import composite_ref as cr

PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "composite_reference_cpu_float32.json")
K_BAR = json.load(open(PROFILE))["K"]
TILE = cr.TILE
SLACK = 37                                # slots of every frame past the fullest frame's pairs
NONFINITE_ROWS = np.arange(150, 166)      # hard_64x48: NaN / inf conic or uv
F32 = np.float32


# ------------------------------------------------------------------ clips
@dataclasses.dataclass
class Clip:
    name: str
    W: int
    H: int
    P: int
    frames: list                # composite_ref.Scene per frame
    opacity_per_frame: bool

    @property
    def F(self):
        return len(self.frames)

    @property
    def T(self):
        return ((self.W + TILE - 1) // TILE) * ((self.H + TILE - 1) // TILE)

    def sub(self, which):
        """the clip of the frames ``which`` (the scenes keep their names: their references are shared)"""
        return Clip(f"{self.name}[{','.join(str(f) for f in which)}]", self.W, self.H, self.P, [self.frames[f] for f in which],
                    self.opacity_per_frame)


def tile_counts(uv, radius, W, H):
    """tiles of every splat's rectangle as the sort counts them: (c -+ r) / 16 in float32, truncated toward zero, clamped to the
    grid; radius 0: in no list"""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    u, v = uv[:, 0].astype(F32), uv[:, 1].astype(F32)
    r = np.asarray(radius).reshape(-1).astype(F32)
    with np.errstate(all="ignore"):
        lo = lambda c, g: np.clip(np.trunc((c - r) / F32(TILE)), 0, g)
        hi = lambda c, g: np.clip(np.trunc((((c + r) + F32(TILE)) - F32(1)) / F32(TILE)), 0, g)
        n = (hi(v, gy) - lo(v, gy)) * (hi(u, gx) - lo(u, gx))
    return np.where(r == 0, 0, n).astype(np.int64)


def derive(o, base: cr.Scene, name, uv=None, sort_uv=None, conic=None, opacity=None, depth=None, cull=()) -> cr.Scene:
    """a frame derived from ``base``: other operands, f0's radii after culling and pruning (and without the ids ``cull``), the tile
    counts of the moved centres, pruned to a fixed point"""
    uv = base.uv if uv is None else uv
    sort_uv = base.sort_uv if sort_uv is None else sort_uv
    conic = base.conic if conic is None else conic
    opacity = base.opacity if opacity is None else opacity
    depth = base.depth if depth is None else depth
    W, H = base.W, base.H
    rdt, tdt, tshape = base.radius.dtype, base.tiles.dtype, base.tiles.shape
    assert np.array_equal(tile_counts(base.sort_uv, base.radius, W, H), base.tiles.reshape(-1)), "tile_counts is not the sort's count"
    full = tile_counts(sort_uv, base.radius, W, H)
    live = lambda r: np.where(np.asarray(r).reshape(-1) == 0, 0, full).reshape(tshape).astype(tdt)
    sort = lambda r: o.sort_gaussian(sort_uv, depth, W, H, r.astype(rdt), live(r))
    radius0 = base.radius.copy()
    radius0.reshape(-1)[list(cull)] = 0
    pruned, passes, radius, (idx, tr), wk = cr.prune(uv, conic, opacity, depth, radius0, full, W, H, sort, bias=None)
    cr._WALKS[(name, 0, False)] = wk
    return cr.Scene(name, W, H, base.N, uv, conic, opacity, sort_uv, depth, radius.astype(rdt), live(radius), idx, tr,
                    np.concatenate([base.culled, np.asarray(cull, np.int64)]), pruned, passes, None)


def empty_frame(base: cr.Scene, name) -> cr.Scene:
    """every radius 0: no pair, every tile's list empty"""
    T = ((base.W + TILE - 1) // TILE) * ((base.H + TILE - 1) // TILE)
    return cr.Scene(name, base.W, base.H, base.N, base.uv, base.conic, base.opacity, base.sort_uv, base.depth,
                    np.zeros_like(base.radius), np.zeros_like(base.tiles), np.zeros(0, np.int32), np.zeros((T, 2), np.int32),
                    np.zeros(0, np.int64), np.zeros(0, np.int64), [0], None)


def mirrored(o, base, name):
    W = F32(base.W)
    uv, suv, conic = base.uv.copy(), base.sort_uv.copy(), base.conic.copy()
    uv[:, 0] = W - uv[:, 0]
    suv[:, 0] = W - suv[:, 0]
    conic[:, 1] = -conic[:, 1]
    return derive(o, base, name, uv=uv, sort_uv=suv, conic=conic, opacity=(base.opacity * F32(0.8)).astype(F32))


def reversed_depth(o, base, name, cull=()):
    d = base.depth.astype(F32)
    return derive(o, base, name, depth=((d.max() + d.min()) - d).astype(F32), cull=cull)


_CLIPS = {}


def clip(o, name) -> Clip:
    """the clips by name, built once per session: opaque_x4, hard_x2"""
    if name not in _CLIPS:
        if name == "opaque_x4":
            f0 = cr.scene(o, "opaque_100x60")
            frames = [f0, empty_frame(f0, "opaque_x4_f1_empty"), mirrored(o, f0, "opaque_x4_f2_mirror"),
                      reversed_depth(o, f0, "opaque_x4_f3_revdepth")]
            _CLIPS[name] = Clip(name, f0.W, f0.H, f0.N, frames, True)
        elif name == "hard_x2":
            f0 = cr.scene(o, "hard_64x48")
            # With every Gaussian of f0 in the reversed lists the float32 restatement of Gaussian 304's conic row reaches 0.15 of its
            # companion (4 x 0.15 > K = 0.5; every other row stays below 0.06): the frame is changed, not K -- 304 is in no list of f1
            _CLIPS[name] = Clip(name, f0.W, f0.H, f0.N, [f0, reversed_depth(o, f0, "hard_x2_f1_revdepth", cull=(304,))], False)
        else:
            raise KeyError(name)
    return _CLIPS[name]


# ------------------------------------------------------------------ seeded inputs
def features(cl: Clip, C, per_frame, seed=0):
    """[F,P,C] float32 in [0, 1): another table per frame (frame 0: the table of composite_ref's own cases,
    test_composite_ref_cpu.case_inputs), or that one table for all frames"""
    if per_frame:
        return np.stack([np.random.default_rng(1000 + C + 7919 * f + seed).uniform(size=(cl.P, C)) for f in range(cl.F)]).astype(F32)
    t = np.random.default_rng(1000 + C + seed).uniform(size=(cl.P, C)).astype(F32)
    return np.broadcast_to(t, (cl.F, cl.P, C))


def upstream(cl: Clip, C, kind="normal", seed=0):
    """[F,C,H,W] float32: a seeded normal image per frame; "pixel": on one pixel per tile only, another place in every tile and frame"""
    g = np.stack([np.random.default_rng(3000 + C + 104729 * f + seed).normal(size=(C, cl.H, cl.W)) for f in range(cl.F)]).astype(F32)
    if kind == "pixel":
        m = np.zeros((cl.F, cl.H, cl.W), bool)
        gx, gy = (cl.W + 15) // 16, (cl.H + 15) // 16
        for f in range(cl.F):
            for t in range(gx * gy):
                x0, y0 = 16 * (t % gx), 16 * (t // gx)
                nx, ny = min(16, cl.W - x0), min(16, cl.H - y0)
                m[f, y0 + (5 * t + 3 + f) % ny, x0 + (7 * t + 1 + 2 * f) % nx] = True
        g = g * m[:, None]
    return g


# ------------------------------------------------------------------ references, once per session
_REF = {}


def forward_ref(sc, key, feat, bg, K=0, trunc=False):
    """(walk, image [C,H,W], companion); ``key`` names the feature table"""
    k = ("fwd", sc.name, key, np.asarray(bg, np.float64).tobytes(), K, trunc)
    if k not in _REF:
        wk = cr.scene_walk(sc, K, trunc)
        assert wk.unclear_ids().size == 0, sc.name
        _REF[k] = (wk,) + cr.forward(wk, feat, bg)
    return _REF[k]


def backward_ref(sc, key, feat, bg, g):
    """(grads, comps) of composite_ref.backward on the scene's K = 0 walk; ``key`` names features and upstream gradient"""
    k = ("bwd", sc.name, key, np.asarray(bg, np.float64).tobytes())
    if k not in _REF:
        _REF[k] = cr.backward(cr.scene_walk(sc), sc.conic, sc.opacity, feat, bg, g)
    return _REF[k]


def ratio(got, ref, comp, K):
    return cr.worst_ratio(np.asarray(got), np.asarray(ref, np.float64), K * np.asarray(comp, np.float64))


def check_forward_frame(sc, wk, img, cimg, out, final_T, ncontrib, gs_idx=None):
    """one frame of a forward against its float64 walk: integers exact, ratios returned"""
    fT, nc, gi = wk.image_maps()
    ncontrib = np.asarray(ncontrib)
    assert np.array_equal(ncontrib, nc), f"{sc.name}: ncontrib differs on {int((ncontrib != nc).sum())} pixels"
    if gs_idx is not None:
        gs_idx = np.asarray(gs_idx)
        assert np.array_equal(gs_idx, gi), f"{sc.name}: gs_idx differs on {int((gs_idx != gi).any(-1).sum())} pixels"
    return dict(image=ratio(out, img, cimg, K_BAR["image"]), final_T=ratio(final_T, fT, wk.final_T_companion(), K_BAR["final_T"]))


def check_grads_frame(sc, got, grads, comps, nonfinite=None):
    """one frame's per-Gaussian gradient rows (name -> [P, k]; "tap" is compared with the uv reference given under "tap") against
    the float64 backward: every row of finite operands within K x companion; the rows of the hard scene's non-finite operands are
    left out and what was written there is recorded in ``nonfinite``.  Returns name -> worst ratio."""
    finite = np.ones(sc.N, bool)
    if sc.name.startswith("hard"):
        finite[NONFINITE_ROWS] = False
        if nonfinite is not None:
            for name, a in got.items():
                rows = np.asarray(a).reshape(sc.N, -1)[NONFINITE_ROWS]
                nonfinite[name] = dict(nan=int(np.isnan(rows).sum()), inf=int(np.isinf(rows).sum()),
                                       nonzero=int((np.nan_to_num(rows) != 0).sum()), elements=int(rows.size))
    r = {}
    for name, a in got.items():
        kname = "uv" if name == "tap" else name
        a = np.asarray(a).reshape(sc.N, -1)[finite]
        r[name] = ratio(a, grads[name].reshape(sc.N, -1)[finite], comps[name].reshape(sc.N, -1)[finite], K_BAR[kname])
    return r


def zero_refs(N, C):
    """the gradients of a frame without pairs: all-zero rows, zero companions (any non-zero element is outside)"""
    shp = dict(uv=(N, 2), conic=(N, 3), opacity=(N,), feature=(N, C), abs_uv=(N, 2), tap=(N, 2))
    return {k: np.zeros(s) for k, s in shp.items()}, {k: np.zeros(s) for k, s in shp.items()}


# ------------------------------------------------------------------ records on the host (the CPU tests' stand-in for the tile kernels)
def host_pair_map(sc, cap):
    """a pair map of the frame's lists: Gaussian i owns the slots [goff[i-1], goff[i]) in the order of its tiles; slot [n] of every
    sorted position"""
    idx = np.asarray(sc.idx).reshape(-1).astype(np.int64)
    cnt = np.bincount(idx, minlength=sc.N)
    goff = np.cumsum(cnt).astype(np.int64)
    assert goff[-1] <= cap
    order = np.argsort(idx, kind="stable")
    slot = np.empty(idx.size, np.int64)
    slot[order] = np.arange(idx.size)
    return goff, slot


def host_records(sc, feat, bg, g, layout, cap):
    """[cap, stride] float32 plain records of one frame from the float64 backward of every tile on its own (NaN: unowned slots and
    padding floats), with its pair map"""
    wk = cr.scene_walk(sc)
    goff, slot = host_pair_map(sc, cap)
    rec = np.full((cap, layout["stride"]), np.nan, F32)
    ng, C = layout["ng"], layout["C"]
    rec[:int(goff[-1]), :ng + C] = 0
    for t in wk.tiles:
        if t.ids.size == 0:
            continue
        gr, _ = cr.backward(dataclasses.replace(wk, tiles=[t]), sc.conic, sc.opacity, feat, bg, g, companions=False)
        s = slot[int(sc.tr[t.tile][0]):int(sc.tr[t.tile][0]) + t.ids.size]
        with np.errstate(all="ignore"):
            rec[s, 0:2], rec[s, 2:5], rec[s, 5] = gr["uv"][t.ids], gr["conic"][t.ids], gr["opacity"][t.ids]
            if layout["abs"]:
                rec[s, 6:8] = gr["abs_uv"][t.ids]
            rec[s, ng:ng + C] = gr["feature"][t.ids]
    return rec, goff


def host_segment_sum(rec_flat, start, stride, goff):
    """numpy twin of splat_pair_records_segment_sum: records from float index ``start`` of the flat buffer"""
    P = goff.size
    n = int(goff[-1])
    r = rec_flat[start:start + n * stride].reshape(n, stride).astype(np.float64)
    owner = np.repeat(np.arange(P), np.diff(np.concatenate([[0], goff])))
    out = np.zeros((P, stride))
    np.add.at(out, owner, r)
    return out


def slice_record_sums(S, layout):
    """[P, stride] summed records -> name -> rows, by the layout"""
    ng, C = layout["ng"], layout["C"]
    out = dict(uv=S[:, 0:2], conic=S[:, 2:5], opacity=S[:, 5], feature=S[:, ng:ng + C])
    if layout["abs"]:
        out["abs_uv"] = S[:, list(layout["abs"])]
    if layout["kind"] == "sets":
        out["tap"] = S[:, list(layout["tap"])]
    return out


# ------------------------------------------------------------------ driver (device)
def _L():
    import splatter_a_video_amd._lib as L
    return L


def _t():
    import torch
    return torch


def dev(a, device):
    return None if a is None else _t().as_tensor(np.array(a, order="C"), device=device)     # (a copy: a broadcast table is read-only)


def nan(device, *shape):
    return _t().full(shape, float("nan"), dtype=_t().float32, device=device)


def minus(device, *shape, dtype=None):
    return _t().full(shape, -1, dtype=dtype or _t().int32, device=device)


class Batch:
    """a clip on the device, binned and sorted: [F,P,..] operands, tile_range [F,T,2], idx_sorted / slot_sorted [F,capacity],
    goff [F,P]; ``reach``: the reach-masked lists (splat_bin_count_batch_reach / splat_bin_sort_batch_reach)"""

    def __init__(self, cl: Clip, device, reach=False):
        torch, L = _t(), _L()
        lib, st = L.lib(), L.stream
        self.clip, self.dev, self.reach_lists = cl, device, reach
        F, P, W, H, T = cl.F, cl.P, cl.W, cl.H, cl.T
        self.F, self.P, self.W, self.H, self.T = F, P, W, H, T
        stack = lambda k, shape: dev(np.stack([np.asarray(getattr(s, k)).reshape(shape) for s in cl.frames]), device)
        self.uv, self.conic = stack("uv", (P, 2)).float(), stack("conic", (P, 3)).float()
        self.sort_uv, self.depth = stack("sort_uv", (P, 2)).float(), stack("depth", (P, 1)).float()
        self.radius = stack("radius", (P,)).to(torch.int32)
        if cl.opacity_per_frame:
            self.opacity, self.op_fs = stack("opacity", (P,)).float(), P
        else:
            assert all(np.array_equal(s.opacity, cl.frames[0].opacity) for s in cl.frames)
            self.opacity, self.op_fs = dev(cl.frames[0].opacity.reshape(P), device).float(), 0
        scratch = torch.empty(F * int(lib.splat_bin_scratch_bytes(P, W, H)), dtype=torch.uint8, device=device)
        self.tile_range = minus(device, F, T, 2)
        self.M = minus(device, F)
        self.reach = minus(device, F, P) if reach else None
        if reach:
            L.check(lib.splat_bin_count_batch_reach(F, P, L.ptr(self.sort_uv), L.ptr(self.radius), L.ptr(self.conic), L.ptr(self.opacity),
                                                    self.op_fs, W, H, L.ptr(scratch), L.ptr(self.tile_range), L.ptr(self.M), L.ptr(None),
                                                    L.ptr(self.reach), st()))
        else:
            L.check(lib.splat_bin_count_batch(F, P, L.ptr(self.sort_uv), L.ptr(self.radius), W, H, L.ptr(scratch), L.ptr(self.tile_range),
                                              L.ptr(self.M), st()))
        self.pairs = self.M.cpu().numpy().astype(np.int64)
        assert (self.pairs >= 0).all()
        if not reach:
            assert [int(m) for m in self.pairs] == [int(np.asarray(s.idx).size) for s in cl.frames], "pairs per frame differ from the walks'"
        cap = self.cap = int(self.pairs.max()) + SLACK
        self.keys = minus(device, F, cap, dtype=torch.int64)
        self.idx_sorted, self.slot_sorted, self.owner = minus(device, F, cap), minus(device, F, cap), minus(device, F, cap)
        self.goff = minus(device, F, P)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=device)
        tail = (W, H, L.ptr(scratch), L.ptr(self.tile_range), cap, L.ptr(self.keys), L.ptr(self.idx_sorted), L.ptr(self.overflow),
                L.ptr(self.goff), L.ptr(self.owner), L.ptr(self.slot_sorted), st())
        if reach:
            L.check(lib.splat_bin_sort_batch_reach(F, P, L.ptr(self.sort_uv), L.ptr(self.depth), L.ptr(self.radius), L.ptr(self.reach), *tail))
        else:
            L.check(lib.splat_bin_sort_batch(F, P, L.ptr(self.sort_uv), L.ptr(self.depth), L.ptr(self.radius), *tail))
        torch.cuda.synchronize()
        assert int(self.overflow.item()) == 0
        self.h_idx, self.h_tr = self.idx_sorted.cpu().numpy(), self.tile_range.cpu().numpy()
        self.h_goff, self.h_slot = self.goff.cpu().numpy(), self.slot_sorted.cpu().numpy()
        for f, s in enumerate(cl.frames):
            m = int(self.pairs[f])
            assert int(self.h_goff[f, -1]) == m, f"frame {f}: goff_incl ends at {int(self.h_goff[f, -1])}, {m} pairs"
            assert np.array_equal(np.sort(self.h_slot[f, :m]), np.arange(m)), f"frame {f}: slot_sorted is no permutation of the frame's slots"
            if not reach:   # bit-equal to the lists the float64 walks used
                assert np.array_equal(self.h_idx[f, :m], np.asarray(s.idx).reshape(-1)), f"frame {f}: sorted ids differ from the walk's"
                assert np.array_equal(self.h_tr[f], np.asarray(s.tr).reshape(-1, 2)), f"frame {f}: tile ranges differ from the walk's"

    def frame_lists(self, f):
        m = int(self.pairs[f])
        return self.h_idx[f, :m].copy(), self.h_tr[f].copy()


def _sync():
    _t().cuda.synchronize()


def _fwd_buffers(B, C, K, cull, pack_width=None):
    torch, L = _t(), _L()
    d = dict(out=nan(B.dev, B.F, C, B.H, B.W), final_T=nan(B.dev, B.F, B.H, B.W), ncontrib=minus(B.dev, B.F, B.H, B.W),
             gs_idx=torch.full((B.F, B.H, B.W, K), -2, dtype=torch.int32, device=B.dev) if K else None,
             pack=nan(B.dev, B.F * B.P * int(L.lib().splat_blend_pack_floats(pack_width or C))),
             cull=minus(B.dev, B.F, B.cap) if cull else None)
    return d


def forward_batch(B, C, feature, feature_fs, bg=0.0, bgc=None, K=0, trunc=False, cull=True):
    """splat_alpha_blending_forward_batch; feature: device tensor [F,P,C] (feature_fs = P * C) or [P,C] (0)"""
    L = _L()
    o = _fwd_buffers(B, C, K, cull)
    L.check(L.lib().splat_alpha_blending_forward_batch(
        B.F, B.P, C, L.ptr(B.uv), L.ptr(B.conic), L.ptr(B.opacity), B.op_fs, L.ptr(feature), feature_fs, L.ptr(B.idx_sorted),
        L.ptr(B.tile_range), B.cap, float(bg), L.ptr(bgc), B.W, B.H, K, int(trunc), L.ptr(o["out"]), L.ptr(o["final_T"]),
        L.ptr(o["ncontrib"]), L.ptr(o["gs_idx"]), L.ptr(o["pack"]), L.ptr(o["cull"]), L.stream()))
    _sync()
    return o


def source_table(sources):
    """sources: (c0, cn, device tensor, frame stride in floats)"""
    L = _L()
    table = (L.FeatureSource * L.MAX_SOURCES)()
    for n, (c0, cn, t, fs) in enumerate(sources):
        table[n].c0, table[n].cn, table[n].feature, table[n].d_feature, table[n].frame_stride = c0, cn, t.data_ptr(), None, int(fs)
    return table


def forward_batch_sources(B, C, sources, bgc, K=0, trunc=False, cull=True):
    L = _L()
    o = _fwd_buffers(B, C, K, cull)
    L.check(L.lib().splat_alpha_blending_forward_batch_sources(
        B.F, B.P, C, len(sources), source_table(sources), L.ptr(B.uv), L.ptr(B.conic), L.ptr(B.opacity), B.op_fs, L.ptr(B.idx_sorted),
        L.ptr(B.tile_range), B.cap, L.ptr(bgc), B.W, B.H, K, int(trunc), L.ptr(o["out"]), L.ptr(o["final_T"]), L.ptr(o["ncontrib"]),
        L.ptr(o["gs_idx"]), L.ptr(o["pack"]), L.ptr(o["cull"]), L.stream()))
    _sync()
    return o


def set_tables(plan, tensors=None, strides=None):
    """host tables of a three-group plan (c0[3], cn[3], bg[3]); tensors: per group a device tensor or None"""
    i3, f3 = ctypes.c_int32 * 3, ctypes.c_float * 3
    c0, cn, bg = plan
    ptrs = (ctypes.c_void_p * 3)(*[0 if t is None else t.data_ptr() for t in (tensors or [None] * 3)])
    return dict(c0=i3(*c0), cn=i3(*cn), bg=f3(*bg), ptr=ptrs, fs=(ctypes.c_int64 * 3)(*(strides or [0, 0, 0])))


def forward_batch_sets(B, C, plan, tensors, strides, bgc, K=0, trunc=False, cull=True):
    L = _L()
    o = _fwd_buffers(B, C, K, cull)
    tb = set_tables(plan, tensors, strides)
    L.check(L.lib().splat_alpha_blending_forward_batch_sets(
        B.F, B.P, C, tb["c0"], tb["cn"], tb["ptr"], tb["fs"], L.ptr(B.uv), L.ptr(B.conic), L.ptr(B.opacity), B.op_fs,
        L.ptr(B.idx_sorted), L.ptr(B.tile_range), B.cap, L.ptr(bgc), B.W, B.H, K, int(trunc), L.ptr(o["out"]), L.ptr(o["final_T"]),
        L.ptr(o["ncontrib"]), L.ptr(o["gs_idx"]), L.ptr(o["pack"]), L.ptr(o["cull"]), L.stream()))
    _sync()
    return o


def backward_batch(B, C, fw, dL, bg, want_abs, cull=True):
    """splat_alpha_blending_backward_batch from what a forward left -> (records [F * capacity * stride], stride)"""
    L = _L()
    stride = int(L.lib().splat_blend_pair_stride(C, 1 if want_abs else 0, 0))
    rec = nan(B.dev, B.F * B.cap * stride)
    L.check(L.lib().splat_alpha_blending_backward_batch(
        B.F, B.P, C, L.ptr(B.idx_sorted), L.ptr(B.tile_range), B.cap, float(bg), B.W, B.H, L.ptr(fw["final_T"]), L.ptr(fw["ncontrib"]),
        L.ptr(dL), 1 if want_abs else 0, L.ptr(B.slot_sorted), L.ptr(rec), L.ptr(fw["pack"]), L.ptr(fw["cull"] if cull else None),
        L.ptr(None), L.stream()))
    _sync()
    return rec, stride


def backward_batch_sets(B, C, plan, fw, want_abs, feature=None, feature_fs=0, set_feature=None, set_fs=None, dL=None, set_dL=None,
                        cull=True, forward_pack=None, packed=True, l1=None):
    """splat_alpha_blending_backward_batch_sets / _sets_packed / (l1 = dict(pred, targets[3], scale[3], sums)) _sets_l1"""
    L = _L()
    lib = L.lib()
    stride = int(lib.splat_blend_sets_pair_stride(C))
    rec = nan(B.dev, B.F * B.cap * stride)
    scratch = nan(B.dev, B.F * B.P * int(lib.splat_blend_sets_pack_floats()))
    tb = set_tables(plan, set_feature, set_fs)
    sf = (tb["ptr"], tb["fs"]) if set_feature is not None else (None, None)
    if set_feature is None and feature is None:      # a row described by sources: the table is given, its pointers are NULL
        sf = (tb["ptr"], tb["fs"])
    dl = None if set_dL is None else (ctypes.c_void_p * 3)(*[0 if t is None else t.data_ptr() for t in set_dL])
    head = (B.F, B.P, C, tb["c0"], tb["cn"], tb["bg"], L.ptr(B.uv), L.ptr(B.conic), L.ptr(B.opacity), B.op_fs)
    lists = (L.ptr(B.idx_sorted), L.ptr(B.tile_range), B.cap, B.W, B.H, L.ptr(fw["final_T"]), L.ptr(fw["ncontrib"]))
    tail = (1 if want_abs else 0, L.ptr(B.slot_sorted), L.ptr(rec), L.ptr(scratch), L.ptr(fw["cull"] if cull else None), L.ptr(None))
    if l1 is not None:
        tg = (ctypes.c_void_p * 3)(*[0 if t is None else t.data_ptr() for t in l1["targets"]])
        L.check(lib.splat_alpha_blending_backward_batch_sets_l1(
            *head, sf[0], sf[1], *lists, L.ptr(l1["pred"]), tg, (ctypes.c_float * 3)(*l1["scale"]), L.ptr(l1["sums"]), *tail,
            L.ptr(forward_pack), L.stream()))
    elif packed:
        L.check(lib.splat_alpha_blending_backward_batch_sets_packed(
            *head, L.ptr(feature), feature_fs, sf[0], sf[1], *lists, L.ptr(dL), dl, *tail, L.ptr(forward_pack), L.stream()))
    else:
        assert forward_pack is None
        L.check(lib.splat_alpha_blending_backward_batch_sets(
            *head, L.ptr(feature), feature_fs, sf[0], sf[1], *lists, L.ptr(dL), dl, *tail, L.stream()))
    _sync()
    return rec, stride


def forward_batch_set(B, C, c0, cn, feature, feature_fs, bg, out, cull=True):
    """one chunk of a wide set into channels [c0, c0 + cn) of ``out`` [F,C,H,W]; the chunk's own final_T / ncontrib / pack / cull"""
    L = _L()
    o = _fwd_buffers(B, 1, 0, cull, pack_width=cn)
    o["out"] = out
    L.check(L.lib().splat_alpha_blending_forward_batch_set(
        B.F, B.P, C, c0, cn, L.ptr(B.uv), L.ptr(B.conic), L.ptr(B.opacity), B.op_fs, L.ptr(feature), feature_fs, L.ptr(B.idx_sorted),
        L.ptr(B.tile_range), B.cap, float(bg), B.W, B.H, L.ptr(out), L.ptr(o["final_T"]), L.ptr(o["ncontrib"]), L.ptr(o["pack"]),
        L.ptr(o["cull"]), L.stream()))
    _sync()
    return o


def backward_batch_set_packed(B, C, c0, cn, fw, dL, bg, cull=True):
    L = _L()
    stride = int(L.lib().splat_blend_pair_stride(cn, 0, 0))
    rec = nan(B.dev, B.F * B.cap * stride)
    L.check(L.lib().splat_alpha_blending_backward_batch_set_packed(
        B.F, B.P, C, c0, cn, L.ptr(B.idx_sorted), L.ptr(B.tile_range), B.cap, float(bg), B.W, B.H, L.ptr(fw["final_T"]),
        L.ptr(fw["ncontrib"]), L.ptr(dL), L.ptr(B.slot_sorted), L.ptr(rec), L.ptr(fw["pack"]), L.ptr(fw["cull"] if cull else None),
        L.ptr(None), L.stream()))
    _sync()
    return rec, stride


def backward_batch_set(B, C, c0, cn, feature, feature_fs, fw, dL, bg, want_abs):
    """packs its own records from the inputs; no cull words"""
    L = _L()
    stride = int(L.lib().splat_blend_pair_stride(cn, 1 if want_abs else 0, 0))
    rec = nan(B.dev, B.F * B.cap * stride)
    scratch = nan(B.dev, B.F * B.P * int(L.lib().splat_blend_pack_floats(cn)))
    L.check(L.lib().splat_alpha_blending_backward_batch_set(
        B.F, B.P, C, c0, cn, L.ptr(B.uv), L.ptr(B.conic), L.ptr(B.opacity), B.op_fs, L.ptr(feature), feature_fs, L.ptr(B.idx_sorted),
        L.ptr(B.tile_range), B.cap, float(bg), B.W, B.H, L.ptr(fw["final_T"]), L.ptr(fw["ncontrib"]), L.ptr(dL), 1 if want_abs else 0,
        L.ptr(B.slot_sorted), L.ptr(rec), L.ptr(scratch), L.ptr(None), L.stream()))
    _sync()
    return rec, stride


def reduce_frames(B, rec, stride, shift=0):
    """per frame [P, stride] float32: splat_pair_records_segment_sum over frame f's records at (f * capacity + shift) * stride with
    goff_incl[f]"""
    L = _L()
    out = []
    flat = rec.view(-1)
    for f in range(B.F):
        o = nan(B.dev, B.P, stride)
        start = (f * B.cap + shift) * stride
        L.check(L.lib().splat_pair_records_segment_sum(B.P, stride, L.ptr(flat[start:]), L.ptr(B.goff[f]), L.ptr(o), L.stream()))
        _sync()
        out.append(o.cpu().numpy())
    return out


# ------------------------------------------------------------------ feature sets of one row (the one-pass backward's plans)
# name -> (first row channel, width, background) of the three routing groups: tap set | second live set | detached set
PLANS = {"3|1|19": ((0, 3, 4), (3, 1, 19), (0.25, 1.0, 0.0)), "3|-|10": ((0, 0, 3), (3, 0, 10), (0.25, 0.0, 0.0)),
         "3|1|4": ((0, 3, 4), (3, 1, 4), (0.25, 1.0, 0.0)), "3|1|8": ((0, 3, 4), (3, 1, 8), (0.25, 1.0, 0.0)),
         "3|1|9": ((0, 3, 4), (3, 1, 9), (0.25, 1.0, 0.0))}


def plan_bgc(plan):
    c0, cn, bg = plan
    out = np.zeros(sum(cn), F32)
    for g in range(3):
        out[c0[g]:c0[g] + cn[g]] = bg[g]
    return out


def sets_inputs(cl: Clip, name):
    """per group the features [F,P,w] (group 1, the depth's place, has another table per frame; the others are shared) and the
    upstream gradient [F,w,H,W]; None for a group without channels"""
    c0, cn, _ = PLANS[name]
    seed = 50000 + 131 * sum(cn)
    feats = [None if not w else features(cl, w, g == 1, seed + g) for g, w in enumerate(cn)]
    gims = [None if not w else upstream(cl, w, "normal", seed + 10 + g) for g, w in enumerate(cn)]
    return feats, gims


def sets_row(cl, name, parts):
    """the groups' arrays [F, .., w] laid into the row's channels (axis -1 for features, 1 for images)"""
    c0, cn, _ = PLANS[name]
    order = sorted((c0[g], g) for g in range(3) if cn[g])
    axis = -1 if parts[order[0][1]].ndim == 3 else 1
    return np.ascontiguousarray(np.concatenate([parts[g] for _, g in order], axis=axis))


def sets_ref(cl: Clip, f, name, feats, gims, key="sets"):
    """frame f's summed reference of a plan (uv, conic <- every set; opacity <- the live sets; abs_uv, tap <- the tap set; feature
    = the row's channels) with the summed companions"""
    sc = cl.frames[f]
    c0, cn, bg = PLANS[name]
    C = sum(cn)
    tot, ctot = zero_refs(sc.N, C)
    for g in range(3):
        if not cn[g]:
            continue
        gr, cp = backward_ref(sc, (key, name, g), feats[g][f], bg[g], gims[g][f])
        for k in ("uv", "conic"):
            tot[k], ctot[k] = tot[k] + gr[k], ctot[k] + cp[k]
        if g != 2:
            tot["opacity"], ctot["opacity"] = tot["opacity"] + gr["opacity"], ctot["opacity"] + cp["opacity"]
        if g == 0:
            tot["abs_uv"], ctot["abs_uv"] = gr["abs_uv"], cp["abs_uv"]
            tot["tap"], ctot["tap"] = gr["uv"], cp["uv"]
        tot["feature"][:, c0[g]:c0[g] + cn[g]], ctot["feature"][:, c0[g]:c0[g] + cn[g]] = gr["feature"], cp["feature"]
    return tot, ctot


def l1_target(img, cimg, seed):
    """target = float64 image + s (0.05 + 2 K_image companion), a seeded sign s per element, as float32: (target, s).  Every
    prediction within the image bar has sign(pred - target) = -s (tests/test_frames_composite_ref_cpu.py)."""
    s = np.random.default_rng(seed).choice([-1.0, 1.0], size=img.shape)
    return (img + s * (0.05 + 2.0 * K_BAR["image"] * cimg)).astype(F32), s
