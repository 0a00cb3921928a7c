"""The frame batch's Gaussian-side backward (frames_gauss_bwd_static_kernel / frames_gauss_bwd_dynamic_kernel,
csrc/preprocess.hip) on its own: pair records built here (no compositor), the float64 answer = segment sums of the records
fed to the float64 twin's chain (geometry_ref.chain_ref), and thin ctypes callers of the library's entry points.  Shared by
tests/test_gauss_backward_ref_cpu.py (builder invariants, the float32 C oracle inside the bars) and
tests/test_gpu_gauss_backward_reference.py (the HIP kernels).  No GPU call at import.

Records hold k / 256 with integer |k| <= 256 (the abs sums ax ay >= 0).  A Gaussian owns at most 34 * 19 + 300 < 2^14
records of a batch, so every sum is a multiple of 2^-8 below 2^14: exact in float32 in ANY order -- the kernels' sums are
compared bit for bit.  Every slot no Gaussian owns and every padding float of a record is NaN: an output that depends on
one of them shows it.

Which (frame, row) pairs receive records for the chain comparisons: the kernels make no cull decision -- a record means
"visible with a radius" -- so the float64 reference decides: not culled, EWA ok with a non-empty tile rectangle (the
twin's conic is zero otherwise), kappa < KAPPA_DEAD; rows within the float32 margin of a cull bound, of the radius' ceil
or of a tile rectangle's floor get none either, because the float32 C oracle that proves the bars attainable (unlike the
kernels) makes those decisions itself.  Every other pair has count 0 and its expected contribution is exactly zero; no
row leaves any comparison.

Chain bar of a row (geometry_ref's gradient bar, nothing new): |a - b| <= 2e-3 |b| + 1e-4 rowscale, rowscale = the
maximum of rowmax|b| and the sum over the contributing frames f of widen(kappa_f) * max(rowmax|b_f|, nat_f) -- nat_f the
natural size |g_f| |J_f| of frame f's gradient as in geometry_ref.chain_ref, widened only for gradients that pass through
the conic.  With ``accumulate`` onto a pre-fill v: + 2^-24 |v + b| (one float32 addition).
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

import geometry_ref as gr
import torch_twin as tw

CYCLE = (0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 18, 19)   # both sides of U = 6 / TAIL = 6 (narrow) and of U = 2 / TAIL = 4 (wide)
LONG = 300            # records of the two long rows (50 tail rounds)
SLACK = 5             # slots of every frame past its last pair: owned by no Gaussian
ZERO_ROW = 12         # (P >= 63) no record in any frame
SETS_NG = 12
PLAN23 = dict(C=23, c0=(0, 3, 4), cn=(3, 1, 19), depth_channel=3)   # the renderer's plan: rgb 0-2 | depth 3 | attributes 4-22
W_H = (17, 33)        # image size of the o257 / p257 cases
LINEAR_P = (1, 63, 64, 65, 257)
LINEAR_F = (1, 2, 3, 4, 5, 33, 34)


def lib():
    import splatter_a_video_amd._lib as L
    return L


# ------------------------------------------------------------------ layouts
def plain_layout(C, want_abs):
    """[ux uy ca cb cc o | ax ay (abs) | features], padded to 16-byte chunks"""
    ng = 8 if want_abs else 6
    stride = int(lib().lib().splat_blend_pair_stride(C, 1 if want_abs else 0, 0))
    used = list(range(ng + C))
    assert stride % 4 == 0 and stride >= len(used)
    return dict(kind="plain", C=C, want_abs=bool(want_abs), ng=ng, stride=stride, used=used, nonneg=[6, 7] if want_abs else [],
                tap=(0, 1), abs=(6, 7) if want_abs else None)


def sets_layout(C):
    """[ux uy ca cb | cc o ax ay | tx ty 0 0 | row channels]"""
    stride = int(lib().lib().splat_blend_sets_pair_stride(C))
    used = list(range(10)) + list(range(SETS_NG, SETS_NG + C))
    assert stride % 4 == 0 and stride >= SETS_NG + C
    return dict(kind="sets", C=C, want_abs=True, ng=SETS_NG, stride=stride, used=used, nonneg=[6, 7], tap=(8, 9), abs=(6, 7))


def plain_strides():
    """every stride the library hands out for plain records (C <= 32, with and without the abs sums)"""
    L = lib().lib()
    return sorted({int(L.splat_blend_pair_stride(C, a, 0)) for C in range(1, 33) for a in (0, 1)})


def sets_strides():
    L = lib().lib()
    return sorted({int(L.splat_blend_sets_pair_stride(C)) for C in range(1, 29)})


# ------------------------------------------------------------------ counts and records
def count_table(F, P):
    """[F, P] records per (frame, Gaussian): the cycle of CYCLE shifted from frame to frame, two rows with LONG records in one
    frame (the first and the last frame: at F >= 33 a frame whose slot range is read from global memory), one row without any,
    and a record in every frame for the first and the last Gaussian of every block of 64 (LDS entry 0 of a workgroup is the last
    Gaussian of the workgroup before)"""
    f, i = np.arange(F)[:, None], np.arange(P)[None, :]
    cnt = np.asarray(CYCLE)[(i + 5 * f) % len(CYCLE)]
    edge = (i % 64 == 0) | (i % 64 == 63) | (i == P - 1)
    cnt = np.where(edge & (cnt == 0), 7, cnt)
    if P >= 63:
        cnt[:, ZERO_ROW] = 0
        cnt[0, 2] = LONG
        cnt[F - 1, P - 3] = LONG
    return cnt.astype(np.int64)


def build_records(cnt, layout, seed=0, wide_range=False):
    """goff_incl [F,P] int32, capacity, pair_records [F, capacity, stride] float32 (NaN: unowned slots and padding floats),
    owner [F, capacity] (-1: unowned)"""
    F, P = cnt.shape
    goff = np.cumsum(cnt, axis=1).astype(np.int32)
    cap = int(goff[:, -1].max()) + SLACK
    owner = np.full((F, cap), -1, np.int64)
    for f in range(F):
        owner[f, :goff[f, -1]] = np.repeat(np.arange(P), cnt[f])
    rng = np.random.default_rng(4000 + seed)
    used = layout["used"]
    if wide_range:
        v = np.exp(rng.uniform(np.log(1e-6), np.log(1e3), size=(F, cap, len(used)))) * rng.choice([-1.0, 1.0], size=(F, cap, len(used)))
    else:
        v = rng.integers(-256, 257, size=(F, cap, len(used))) / 256.0
    for k in layout["nonneg"]:
        v[:, :, used.index(k)] = np.abs(v[:, :, used.index(k)])
    rec = np.full((F, cap, layout["stride"]), np.nan, np.float32)
    rec[:, :, used] = v.astype(np.float32)
    rec[owner < 0] = np.nan
    return dict(F=F, P=P, cnt=cnt, goff=goff, cap=cap, rec=rec, owner=owner, layout=layout)


def segment_sums(R, absolute=False):
    """float64 [F, P, stride]: per frame the sum of every Gaussian's records (padding columns: 0)"""
    F, P, lay = R["F"], R["P"], R["layout"]
    out = np.zeros((F, P, lay["stride"]))
    for f in range(F):
        own = R["owner"][f] >= 0
        v = R["rec"][f][own][:, lay["used"]].astype(np.float64)
        tmp = np.zeros((P, len(lay["used"])))
        np.add.at(tmp, R["owner"][f][own], np.abs(v) if absolute else v)
        out[f][:, lay["used"]] = tmp
    return out


def feature_sums(R, S=None):
    """[F, P, C] of the row's channels"""
    S = segment_sums(R) if S is None else S
    ng, C = R["layout"]["ng"], R["layout"]["C"]
    return S[:, :, ng:ng + C]


def taps(R, S, W, H, cols):
    s = S[:, :, list(cols)].sum(0)
    return (s * np.array([0.5 * W, 0.5 * H])).astype(np.float32)


def make_radius(F, P, seed=0):
    return np.random.default_rng(77 + seed).integers(0, 900, size=(F, P)).astype(np.int32)


def prefill(shape, seed, accumulate):
    """store mode: NaN (every element must come back written); add mode: multiples of 2^-8 (sums stay exact)"""
    if not accumulate:
        return np.full(shape, np.nan, np.float32)
    return (np.random.default_rng(300 + seed).integers(-256, 257, size=shape) / 256.0).astype(np.float32)


# ------------------------------------------------------------------ geometry: which (frame, row) pairs get records
def static_frames(cid, F, cam):
    """the F per-frame variants of a geometry case.  cam 0: ONE orthographic camera, positions moved by per-frame offsets (they
    only decide which frames see a row: the kernel's chain runs once, at xyz); 1: an orthographic camera per frame + offsets;
    2: the pinhole camera with per-frame intr / extr / offsets"""
    c = gr.case_by_id(cid)
    assert c["ortho"] == (cam != 2)
    frames = gr.frame_cases(c, F, offsets=True)
    if cam == 0:
        frames = [dict(fc, intr=c["intr"], extr=c["extr"]) for fc in frames]
    return c, frames


def eligible(r):
    """rows of one float64 chain reference that may own records in that frame"""
    _, rows = gr.ewa_rows(r, r["mag_u"], r["mag_v"], r["cull_safe"])
    return (rows & ~r["cull"] & r["live"] & (r["kappa"] < gr.KAPPA_DEAD)).numpy()


@functools.lru_cache(maxsize=None)
def static_eligibility(cid, F, cam):
    c, frames = static_frames(cid, F, cam)
    return np.stack([eligible(gr.chain_ref(fc, offset=True)) for fc in frames])


DYN_TIMES = {
    "single": [7.0],
    "run1": [5.0], "run2": [5.0, 6.0], "run3": [5.0, 6.0, 7.0], "run4": [5.0, 6.0, 7.0, 8.0],
    "run5": [0.0, 1.0, 2.0, 3.0, 4.0], "run9": [float(t) for t in np.linspace(4.5, 7.875, 9)],
    "segments_ABA": [5.0, 6.0, 9.0, 10.0, 11.0, 7.0, 8.0],
    "first_last_knots": [0.0, 4.0, 8.0, 12.0, 16.0, 20.0],
    "frames33": [float(t) for t in np.linspace(0.0, 20.0, 33)],
}
DYN_HARD_ROWS = range(10)   # make_dyn_case: quaternion sums of norm 1e-10 .. 0, opacity logits +-30, scaling logits -12 .. +3


@functools.lru_cache(maxsize=None)
def dyn_case():
    """gr.make_dyn_geom_case("o257") with its ten hard parameter rows moved onto positions the camera sees (in the geometry case
    they sit on the near bound, where half of them are culled in every frame): the rows must receive records"""
    c = gr.make_dyn_geom_case("o257")
    seen = np.stack([eligible(gr.chain_ref(c, dyn=(t, tw.GAUSSIAN_MAJOR))) for t in DYN_TIMES["frames33"]]).all(0)
    donors = np.nonzero(seen & (c["stratum"] == gr.STRATA.index("control")))[0][:10]
    assert donors.size == 10
    pos, cub = c["position"].copy(), c["cubic"].copy()
    pos[:10], cub[:10] = pos[donors], cub[donors]
    return dict(c, position=pos, cubic=cub)


def segments(c, times):
    return [int(c["clock"].scalars(t)[0]) for t in times]


@functools.lru_cache(maxsize=None)
def dyn_eligibility(name):
    c = dyn_case()
    return np.stack([eligible(gr.chain_ref(dict(c, g_opa=np.zeros((c["N"], 1), np.float32)), dyn=(t, tw.GAUSSIAN_MAJOR)))
                     for t in DYN_TIMES[name]])


def frame_table_host(clock, times):
    """the per-frame scalars table of FrameBatch.frame_table (frames.py), on the host: [F, 16] float32"""
    from splatter_a_video_amd.dynamics import _walk_order
    host = np.zeros((len(times), 16), np.float32)
    for f, t in enumerate(times):
        seg, d, basis = clock.scalars(t)
        host[f, 0] = np.array([seg], np.int32).view(np.float32)[0]
        host[f, 1] = d
        host[f, 2:14] = np.frombuffer(basis, dtype=np.float32, count=12)
    _walk_order(host)
    return host


# ------------------------------------------------------------------ float64 reference of the chain outputs
STATIC_OUT = (("d_xyz", "dxyz", "nat_xyz"), ("d_scales", "dscale", "nat_scale"), ("d_uquats", "dquat", "nat_quat"))
DYN_OUT = ("d_position", "d_cubic", "d_rotation", "d_scaling", "d_opacity")


def upstream(R, S, f, depth_channel):
    """the summed records of frame f as the upstream gradients of geometry_ref.chain_ref"""
    ng = R["layout"]["ng"]
    s = S[f]
    g_d = s[:, ng + depth_channel:ng + depth_channel + 1] if depth_channel >= 0 else np.zeros((R["P"], 1))
    return dict(g_uv=s[:, 0:2].astype(np.float32), g_conic=s[:, 2:5].astype(np.float32), g_d=g_d.astype(np.float32),
                g_opa=s[:, 5:6].astype(np.float32))


def _accumulate(tot, name, ref, nat, w):
    ref = ref.reshape(ref.shape[0], -1)
    rs = torch.maximum(torch.nan_to_num(ref).abs().max(1).values, nat) * w
    if name not in tot:
        tot[name] = [torch.zeros_like(ref), torch.zeros_like(rs)]
    tot[name][0] += ref
    tot[name][1] += rs


def _finish(tot):
    out = {}
    for name, (ref, rs) in tot.items():
        out[name] = (ref, gr.grad_bar(ref, rs))
    return out


def static_chain_ref(R, S, frames, cam, depth_channel):
    """{output: (float64 sum over the frames [N, k], bar [N, k])}"""
    tot = {}
    for f, fc in enumerate(frames):
        r = gr.chain_ref(dict(fc, **upstream(R, S, f, depth_channel)), offset=True)
        w = gr.widen(r["kappa"])
        one = torch.ones_like(w)
        for name, key, nat in STATIC_OUT:
            # (the orthographic EWA Jacobian is constant: there the position gradient does not pass through the conic)
            through = cam == 2 if name == "d_xyz" else True
            _accumulate(tot, name, r[key], r[nat], w if through else one)
    return _finish(tot)


def dyn_chain_ref(R, S, c, times, layout, depth_channel):
    tot = {}
    for f, t in enumerate(times):
        r = gr.chain_ref(dict(c, **upstream(R, S, f, depth_channel)), dyn=(t, layout))
        w = gr.widen(r["kappa"])
        one = torch.ones_like(w)
        for name in DYN_OUT:
            _accumulate(tot, name, r[name], r["nat"][name], w if name in ("d_rotation", "d_scaling") else one)
    return _finish(tot)


def check_chain(rep, tag, got, ref, pre=None):
    """``got`` {output: array} against ``ref`` {output: (sum, bar)}; ``pre``: the pre-fill the kernel added onto"""
    for name, (b, bar) in ref.items():
        if pre is not None and pre.get(name) is not None:
            v = gr.T64(pre[name].astype(np.float64)).reshape(b.shape)
            b, bar = v + b, bar + gr.EPS32 * (v + b).abs()
        rep.close(tag + name, got[name], b, bar)


def oracle_static(o, frames, R, S, depth_channel):
    """the float32 C oracle's operator chain per frame on the float32 sums, added up"""
    be = gr.OracleBackend(o)
    tot = {}
    for f, fc in enumerate(frames):
        b = be.fused(dict(fc, **upstream(R, S, f, depth_channel)), True)
        for name, key in (("d_xyz", "dxyz"), ("d_scales", "dscale"), ("d_uquats", "dquat")):
            tot[name] = tot.get(name, 0.0) + np.asarray(b[key], np.float64)
    return tot


def oracle_dynamic(o, c, times, R, S, depth_channel):
    be = gr.OracleBackend(o)
    tot = {}
    for f, t in enumerate(times):
        b = be.frame_preprocess(dict(c, **upstream(R, S, f, depth_channel)), t, tw.GAUSSIAN_MAJOR)
        for name in DYN_OUT:
            tot[name] = tot.get(name, 0.0) + np.asarray(b[name], np.float64).reshape(c["N"], -1)
    return tot


# ------------------------------------------------------------------ ctypes callers (device tensors in, nothing returned)
def dev(a, device):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=device)


def host(t):
    return None if t is None else t.cpu().numpy()


def upload_records(R, device, radius=None):
    """device copies of one record set; every kernel argument below is sized from this ``cap`` and the layout's stride"""
    F, P = R["F"], R["P"]
    rec = dev(R["rec"], device)
    assert rec.numel() == F * R["cap"] * R["layout"]["stride"] and int(R["goff"].max()) <= R["cap"]
    return dict(R, d_rec=rec, d_goff=dev(R["goff"], device), d_radius=dev(radius, device))


def camera_struct(extr, intr=None, offsets=None, per_frame=False):
    from splatter_a_video_amd.frames import _SplatCamera
    c = _SplatCamera()
    c.perspective = 0 if intr is None else 1
    c.intr = None if intr is None else intr.data_ptr()
    c.intr_frame_stride = 4 if (intr is not None and per_frame) else 0
    c.extr = extr.data_ptr()
    c.extr_frame_stride = int(extr.shape[-2] * extr.shape[-1]) if per_frame else 0
    c.offsets = None if offsets is None else offsets.data_ptr()
    return c


def _head(D, W, H, C, with_abs):
    L = lib()
    a = [D["F"], D["P"], C, W, H, D["cap"]]
    if with_abs:
        a.append(1 if D["layout"]["want_abs"] else 0)
    return a + [L.ptr(D["d_rec"]), L.ptr(D["d_goff"]), L.ptr(D["d_radius"])]


def _sync():
    torch.cuda.synchronize()


def _tail(o):
    L = lib()
    return [L.ptr(o.get("tap")), L.ptr(o.get("abs_tap")), L.ptr(o.get("radii_max")), L.stream()]


def _sgrads(o):
    L = lib()
    return [L.ptr(o["d_xyz"]), L.ptr(o["d_scales"]), L.ptr(o["d_uquats"]), L.ptr(o.get("d_opacity"))]


def _sets_tables(sets, o):
    i3 = ctypes.c_int32 * 3
    p3 = (ctypes.c_void_p * 3)(*[0 if o.get(f"set{g}") is None else o[f"set{g}"].data_ptr() for g in range(3)])
    return [i3(*sets["c0"]), i3(*sets["cn"]), p3, i3(*sets["stride"])]


def _source_table(sources, o):
    L = lib()
    table = (L.FeatureSource * L.MAX_SOURCES)()
    for n, s in enumerate(sources):
        table[n].c0, table[n].cn, table[n].feature = s["c0"], s["cn"], None
        buf = o.get(f"src{n}")
        table[n].d_feature = None if buf is None else buf.data_ptr()
        table[n].frame_stride = int(s.get("frame_stride", 0))
    return [len(sources), table]


def call_static(D, g, W, H, o, accumulate=0):
    L = lib()
    C = D["layout"]["C"]
    L.check(L.lib().splat_frames_gauss_backward_static(
        *_head(D, W, H, C, True), L.ptr(g["xyz"]), L.ptr(g["scale"]), L.ptr(g["quat"]), L.ptr(g["extr"]), accumulate,
        *_sgrads(o), L.ptr(o["d_feature"]), *_tail(o)))
    _sync()


def call_static_set(D, g, W, H, o, accumulate=0, feature_stride=None, skip_opacity=0, depth_channel=-1):
    L = lib()
    C = D["layout"]["C"]
    L.check(L.lib().splat_frames_gauss_backward_static_set(
        *_head(D, W, H, C, True), L.ptr(g["xyz"]), L.ptr(g["scale"]), L.ptr(g["quat"]), L.ptr(g["extr"]), accumulate,
        *_sgrads(o), L.ptr(o.get("d_feature")), feature_stride or C, skip_opacity, depth_channel, *_tail(o)))
    _sync()


def call_static_cam(D, g, W, H, o, cam, accumulate=0, feature_stride=None, skip_opacity=0, depth_channel=-1):
    L = lib()
    C = D["layout"]["C"]
    L.check(L.lib().splat_frames_gauss_backward_static_cam(
        *_head(D, W, H, C, True), L.ptr(g["xyz"]), L.ptr(g["scale"]), L.ptr(g["quat"]), ctypes.byref(cam), accumulate,
        *_sgrads(o), L.ptr(o.get("d_feature")), feature_stride or C, skip_opacity, depth_channel, *_tail(o)))
    _sync()


def call_static_sets(D, g, W, H, o, sets, accumulate=0, depth_channel=-1):
    L = lib()
    L.check(L.lib().splat_frames_gauss_backward_static_sets(
        *_head(D, W, H, D["layout"]["C"], False), L.ptr(g["xyz"]), L.ptr(g["scale"]), L.ptr(g["quat"]), L.ptr(g["extr"]),
        accumulate, *_sgrads(o), *_sets_tables(sets, o), depth_channel, *_tail(o)))
    _sync()


def call_static_sets_cam(D, g, W, H, o, cam, sets, accumulate=0, depth_channel=-1):
    L = lib()
    L.check(L.lib().splat_frames_gauss_backward_static_sets_cam(
        *_head(D, W, H, D["layout"]["C"], False), L.ptr(g["xyz"]), L.ptr(g["scale"]), L.ptr(g["quat"]), ctypes.byref(cam),
        accumulate, *_sgrads(o), *_sets_tables(sets, o), depth_channel, *_tail(o)))
    _sync()


def call_static_sources_cam(D, g, W, H, o, cam, sources, accumulate=0, depth_channel=-1):
    L = lib()
    L.check(L.lib().splat_frames_gauss_backward_static_sources_cam(
        *_head(D, W, H, D["layout"]["C"], False), L.ptr(g["xyz"]), L.ptr(g["scale"]), L.ptr(g["quat"]), ctypes.byref(cam),
        accumulate, *_sgrads(o), *_source_table(sources, o), depth_channel, *_tail(o)))
    _sync()


def _dyn_head(D, g, W, H, with_abs):
    L = lib()
    h = _head(D, W, H, D["layout"]["C"], with_abs)
    h.insert(2, g["I"])
    return h + [L.ptr(g["tab"]), L.ptr(g["position"]), L.ptr(g["cubic"]), g["layout"], L.ptr(g["rotation"]),
                L.ptr(g["rot_poly"]), L.ptr(g["rot_fourier"]), L.ptr(g["opacity"]), L.ptr(g["scaling"]), L.ptr(g["extr"])]


def _dgrads(o):
    L = lib()
    return [L.ptr(o.get(k)) for k in ("d_position", "d_cubic", "d_rotation", "d_opacity", "d_scaling")]


def call_dynamic(D, g, W, H, o):
    L = lib()
    L.check(L.lib().splat_frames_gauss_backward_dynamic(*_dyn_head(D, g, W, H, True), *_dgrads(o), L.ptr(o.get("d_feature")), *_tail(o)))
    _sync()


def call_dynamic_sets(D, g, W, H, o, sets, depth_channel=-1):
    L = lib()
    L.check(L.lib().splat_frames_gauss_backward_dynamic_sets(*_dyn_head(D, g, W, H, False), *_dgrads(o), *_sets_tables(sets, o),
                                                             depth_channel, *_tail(o)))
    _sync()


def call_dynamic_sources(D, g, W, H, o, sources, depth_channel=-1):
    L = lib()
    L.check(L.lib().splat_frames_gauss_backward_dynamic_sources(*_dyn_head(D, g, W, H, False), *_dgrads(o),
                                                                *_source_table(sources, o), depth_channel, *_tail(o)))
    _sync()


def call_segment_sum(D, f, out):
    """splat_pair_records_segment_sum over frame f of the record set"""
    L = lib()
    L.check(L.lib().splat_pair_records_segment_sum(D["P"], D["layout"]["stride"], L.ptr(D["d_rec"][f]),
                                                   L.ptr(D["d_goff"][f]), L.ptr(out), L.stream()))
    _sync()


def static_geometry(c, frames, cam, device, P=None):
    """device tensors of a static case's geometry (first P rows) and the camera struct of mode ``cam``"""
    P = c["N"] if P is None else P
    g = dict(xyz=dev(c["xyz"][:P], device), scale=dev(c["scale"][:P], device), quat=dev(c["quat"][:P], device))
    if cam == 0:
        g["extr"] = dev(c["extr"], device)
        g["cam"] = camera_struct(g["extr"])
    else:
        g["extr"] = dev(np.stack([fc["extr"] for fc in frames]), device)
        g["offsets"] = dev(np.stack([fc["offset"][:P] for fc in frames]), device)
        g["intr"] = dev(np.stack([fc["intr"] for fc in frames]), device) if cam == 2 else None
        g["cam"] = camera_struct(g["extr"], g["intr"], g["offsets"], per_frame=True)
    return g


def dyn_geometry(c, times, layout, device, P=None):
    P = c["N"] if P is None else P
    I = c["I"]
    cub = c["cubic"][:P].reshape(P, 4, I, 3)
    cub = np.ascontiguousarray(cub.transpose(2, 0, 1, 3)) if layout == tw.SEGMENT_MAJOR else cub
    g = {k: dev(c[k][:P], device) for k in ("position", "rotation", "rot_poly", "rot_fourier", "opacity", "scaling")}
    g.update(cubic=dev(cub.reshape(-1), device), tab=dev(frame_table_host(c["clock"], times), device), extr=dev(c["extr"], device),
             I=I, layout=layout)
    return g


def cubic_gaussian_major(a, P, I, layout):
    """a d_cubic buffer in the table's layout -> [P, 4 * I * 3] Gaussian-major"""
    a = np.asarray(a)
    return (a.reshape(I, P, 4, 3).transpose(1, 2, 0, 3) if layout == tw.SEGMENT_MAJOR else a).reshape(P, -1)


# ------------------------------------------------------------------ the chain problems (built once, shared by the tests)
CHAIN_F = (1, 3, 5, 34)
CHAIN_CAMS = {0: "o257", 1: "o257", 2: "p257"}
CHAIN_LAYOUTS = ("plain_narrow", "plain_wide", "sets_narrow", "sets_wide")


def chain_layout(key):
    """(layout, depth channel): one narrow (one 16-byte chunk per lane) and one wide stride, each for plain and SETS records"""
    if key == "plain_narrow":
        return plain_layout(3, False), -1
    if key == "plain_wide":
        return plain_layout(20, True), 2
    if key == "sets_narrow":
        return sets_layout(4), 3
    return sets_layout(PLAN23["C"]), PLAN23["depth_channel"]


def layout_sets_tables(lay, depth_channel):
    """three sets that tile the row: [0, d) | the depth channel | the rest"""
    C, d = lay["C"], depth_channel
    return dict(c0=(0, d, d + 1), cn=(d, 1, C - d - 1), stride=(d, 1, max(C - d - 1, 1)))


@functools.lru_cache(maxsize=None)
def static_problem(F, cam, lkey):
    cid = CHAIN_CAMS[cam]
    c, frames = static_frames(cid, F, cam)
    lay, dch = chain_layout(lkey)
    elig = static_eligibility(cid, F, cam)
    R = build_records(count_table(F, c["N"]) * elig, lay, seed=F + 10 * cam)
    S = segment_sums(R)
    case = dict(c, id=f"{cid}.cam{cam}.F{F}.{lkey}")
    return dict(c=case, frames=frames, R=R, S=S, depth_channel=dch, elig=elig, ref=static_chain_ref(R, S, frames, cam, dch))


@functools.lru_cache(maxsize=None)
def dyn_problem(name, lkey):
    c = dyn_case()
    times = DYN_TIMES[name]
    lay, dch = chain_layout(lkey)
    dch = dch if lay["kind"] == "sets" else -1      # (the dynamic kernel takes a depth channel from SETS records only)
    elig = dyn_eligibility(name)
    R = build_records(count_table(len(times), c["N"]) * elig, lay, seed=len(times) + 50)
    S = segment_sums(R)
    case = dict(c, id=f"dyn_o257.{name}.{lkey}")
    return dict(c=case, times=times, R=R, S=S, depth_channel=dch, elig=elig,
                ref=dyn_chain_ref(R, S, c, times, tw.GAUSSIAN_MAJOR, dch))


def report_json(path, backend, reports):
    """worst error / bar per output and case, in the format of profiles/geometry_reference_*.json"""
    import json
    worst = {}
    for rep in reports:
        for (q, s), v in rep.worst.items():
            d = worst.setdefault(rep.case["id"], {}).setdefault(q, {})
            d[s] = max(d.get(s, 0.0), float(f"{v:.4g}"))
    out = dict(backend=backend, what="worst |error| / bar per case, output and stratum (1.0 = on the bar) of the frame batch's "
               "Gaussian-side backward against float64; the linear outputs are compared bit for bit and do not appear",
               constants=dict(KAPPA0=gr.KAPPA0, WIDEN_SLOPE=gr.WIDEN_SLOPE, KAPPA_DEAD=gr.KAPPA_DEAD), worst=worst,
               worst_overall=max(v for c in worst.values() for d in c.values() for v in d.values()))
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return out
