"""The dynamic frame batch's Gaussian-side backward under cameras per frame and the pinhole camera
(frames_gauss_bwd_dynamic_kernel<.., CAM = 1 / 2>, include/splat_hip_views_grad.h) on its own: the problems of
tests/gauss_backward_ref.py (test-built pair records, the float64 chain per frame, geometry_ref's gradient bar) with frame
f under ITS camera.  Shared by tests/test_gauss_backward_cam_ref_cpu.py (the float32 C oracle inside the bars) and
tests/test_gpu_gauss_backward_dynamic_cam.py (the HIP kernel).  No GPU call at import.

Modes: "ortho_pf" = gb.dyn_case() (o257 with dynamic parameters) under gr.camera(W, H, True, f) for frame f: CAM = 1;
"pinhole_pf" = p257 with dynamic parameters under gr.camera(W, H, False, f), extr [F,4,4] and intr [F,4]: CAM = 2;
"pinhole_one" = the same case under its one camera, extr [4,4] and intr [4]: CAM = 2 with both strides 0.

The pinhole case: geometry_ref.make_dyn_geom_case asserts an orthographic case, so its ten lines are restated here.  Its ten
hard parameter rows (quaternion sums of norm 1e-10 .. 0, opacity logits +-30, scaling logits -12 .. +3) are rows 0 .. 9 of the
geometry case, which sit on the near bound; as gb.dyn_case() does for o257, ALL TEN are moved (position and spline) onto
control rows that the case's camera sees at every time of "frames33", so that every time list leaves them records; rows
0 .. 5 (hard rotation / opacity) take the donor's scaling as well, because the pinhole case sizes a splat by its depth.

Bars: gr.grad_bar as in gb.dyn_chain_ref; under the pinhole camera the position gradient passes through the conic (the
Jacobian depends on the point), so gr.widen(kappa) applies to d_position / d_cubic too, as gb.static_chain_ref does for d_xyz
when cam == 2.  No outlier budget.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import gauss_backward_ref as gb
import geometry_ref as gr
import torch_twin as tw

MODES = {"ortho_pf": dict(cid="o257", ortho=True, per_frame=True, cam=1),
         "pinhole_pf": dict(cid="p257", ortho=False, per_frame=True, cam=2),
         "pinhole_one": dict(cid="p257", ortho=False, per_frame=False, cam=2)}
# groups of 1 to 4 frames of one segment, a group cut short by a segment change (the camera follows the frame index, not the
# lane), more than 32 frames
TIMES = ("run1", "run2", "run3", "run4", "run5", "run9", "segments_ABA", "frames33")
# the one-camera pinhole mode differs from "pinhole_pf" in the strides alone: two time lists
ONE_TIMES = ("run5", "segments_ABA")
LINEAR_P = (1, 63, 65, 257)
LINEAR_F = (1, 4, 5, 34)


def problems():
    return [(m, n) for m in ("ortho_pf", "pinhole_pf") for n in TIMES] + [("pinhole_one", n) for n in ONE_TIMES]


def make_dyn_geom_case_any(cid, T=21):
    """gr.make_dyn_geom_case without its orthographic assertion"""
    c = gr.case_by_id(cid)
    d = gr.make_dyn_case(c["N"], T)
    d["id"] = "dyn_" + cid
    d["cubic"] = (d["cubic"] * 0.1).astype(np.float32)
    d.update(position=c["xyz"], scaling=np.log(c["scale"]).astype(np.float32), rotation=c["quat"].copy(), stratum=c["stratum"])
    for k in ("W", "H", "ortho", "intr", "extr", "nearest", "extent", "g_uv", "g_d", "g_conic", "n_edge", "edge_kind"):
        d[k] = c[k]
    return d


@functools.lru_cache(maxsize=None)
def dyn_case(mode):
    if MODES[mode]["ortho"]:
        return gb.dyn_case()
    c = make_dyn_geom_case_any(MODES[mode]["cid"])
    zero = np.zeros((c["N"], 1), np.float32)
    seen = np.stack([gb.eligible(gr.chain_ref(dict(c, g_opa=zero), dyn=(t, tw.GAUSSIAN_MAJOR)))
                     for t in gb.DYN_TIMES["frames33"]]).all(0)
    donors = np.nonzero(seen & (c["stratum"] == gr.STRATA.index("control")))[0][:10]
    assert donors.size == 10
    pos, cub, scl = c["position"].copy(), c["cubic"].copy(), c["scaling"].copy()
    pos[:10], cub[:10] = pos[donors], cub[donors]
    # the pinhole case sizes a splat by its depth (scale = pixels * depth / fx): rows 0 .. 5, whose hard parameter is the
    # rotation or the opacity, take the donor's scaling with its position (row 3 kept the scale of a splat on the near bound
    # and vanished below a pixel at the donor's depth); rows 6 .. 9 keep their hard scaling logits
    scl[:6] = scl[donors[:6]]
    return dict(c, position=pos, cubic=cub, scaling=scl)


def frame_camera(mode, c, f):
    """(intr, extr) of frame f"""
    if not MODES[mode]["per_frame"]:
        return c["intr"], c["extr"]
    return gr.camera(c["W"], c["H"], MODES[mode]["ortho"], f)


def frame_case(mode, c, f):
    intr, extr = frame_camera(mode, c, f)
    return dict(c, intr=intr, extr=extr)


@functools.lru_cache(maxsize=None)
def eligibility(mode, name):
    """[F, N]: rows gb.eligible admits in frame f under frame f's camera"""
    c = dyn_case(mode)
    zero = np.zeros((c["N"], 1), np.float32)
    return np.stack([gb.eligible(gr.chain_ref(dict(frame_case(mode, c, f), g_opa=zero), dyn=(t, tw.GAUSSIAN_MAJOR)))
                     for f, t in enumerate(gb.DYN_TIMES[name])])


def chain_ref(mode, R, S, c, times, depth_channel):
    """{output: (float64 sum over the frames, bar)}: gb.dyn_chain_ref with frame f under its camera"""
    tot = {}
    through_conic = ("d_rotation", "d_scaling") + (("d_position", "d_cubic") if MODES[mode]["cam"] == 2 else ())
    for f, t in enumerate(times):
        r = gr.chain_ref(dict(frame_case(mode, c, f), **gb.upstream(R, S, f, depth_channel)), dyn=(t, tw.GAUSSIAN_MAJOR))
        w = gr.widen(r["kappa"])
        one = w * 0 + 1
        for name in gb.DYN_OUT:
            gb._accumulate(tot, name, r[name], r["nat"][name], w if name in through_conic else one)
    return gb._finish(tot)


@functools.lru_cache(maxsize=None)
def problem(mode, name, lkey):
    c = dyn_case(mode)
    times = gb.DYN_TIMES[name]
    lay, dch = gb.chain_layout(lkey)
    dch = dch if lay["kind"] == "sets" else -1      # (the dynamic kernel takes a depth channel from SETS records only)
    elig = eligibility(mode, name)
    R = gb.build_records(gb.count_table(len(times), c["N"]) * elig, lay, seed=len(times) + 70 + MODES[mode]["cam"])
    S = gb.segment_sums(R)
    case = dict(c, id=f"dyn_{MODES[mode]['cid']}.{mode}.{name}.{lkey}")
    return dict(c=case, mode=mode, times=times, R=R, S=S, depth_channel=dch, elig=elig,
                ref=chain_ref(mode, R, S, c, times, dch))


def oracle_dynamic(o, mode, c, times, R, S, depth_channel):
    """the float32 C oracle per frame -- its dynamic evaluation, its operator chain under the frame's camera, its dynamic
    backward -- added up"""
    be = gr.OracleBackend(o)
    tot = {}
    for f, t in enumerate(times):
        b = be.frame_preprocess(dict(frame_case(mode, c, f), **gb.upstream(R, S, f, depth_channel)), t, tw.GAUSSIAN_MAJOR)
        for name in gb.DYN_OUT:
            tot[name] = tot.get(name, 0.0) + np.asarray(b[name], np.float64).reshape(c["N"], -1)
    return tot


# ------------------------------------------------------------------ device side
def dyn_geometry(mode, c, times, layout, device, P=None):
    """gb.dyn_geometry plus the cameras of the mode: g["cam"] is the splat_camera_t the _cam entry points take"""
    g = gb.dyn_geometry(c, times, layout, device, P)
    cams = [frame_camera(mode, c, f) for f in range(len(times))]
    per_frame = MODES[mode]["per_frame"]
    if per_frame:
        g["extr"] = gb.dev(np.stack([e for _, e in cams]), device)
        g["intr"] = None if MODES[mode]["ortho"] else gb.dev(np.stack([k for k, _ in cams]), device)
    else:
        g["extr"] = gb.dev(c["extr"], device)
        g["intr"] = gb.dev(c["intr"], device)
    g["cam"] = gb.camera_struct(g["extr"], g["intr"], None, per_frame=per_frame)
    return g


def _head(D, g, W, H, with_abs):
    return gb._dyn_head(D, g, W, H, with_abs)[:-1] + [ctypes.byref(g["cam"])]


def call_dynamic_cam(D, g, W, H, o):
    L = gb.lib()
    L.check(L.lib().splat_frames_gauss_backward_dynamic_cam(*_head(D, g, W, H, True), *gb._dgrads(o), L.ptr(o.get("d_feature")),
                                                            *gb._tail(o)))
    gb._sync()


def call_dynamic_sets_cam(D, g, W, H, o, sets, depth_channel=-1):
    L = gb.lib()
    L.check(L.lib().splat_frames_gauss_backward_dynamic_sets_cam(*_head(D, g, W, H, False), *gb._dgrads(o),
                                                                 *gb._sets_tables(sets, o), depth_channel, *gb._tail(o)))
    gb._sync()


def call_dynamic_sources_cam(D, g, W, H, o, sources, depth_channel=-1):
    L = gb.lib()
    L.check(L.lib().splat_frames_gauss_backward_dynamic_sources_cam(*_head(D, g, W, H, False), *gb._dgrads(o),
                                                                    *gb._source_table(sources, o), depth_channel, *gb._tail(o)))
    gb._sync()
