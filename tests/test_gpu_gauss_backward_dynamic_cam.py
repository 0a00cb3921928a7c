"""The dynamic frame batch's Gaussian-side backward under cameras per frame and the pinhole camera
(splat_frames_gauss_backward_dynamic_cam / _sets_cam / _sources_cam, include/splat_hip_views_grad.h: the CAM = 1 and CAM = 2
instantiations of frames_gauss_bwd_dynamic_kernel) called on their own with pair records built by the test, against float64
-- tests/test_gpu_gauss_backward_reference.py::test_dynamic_chain_matches_float64 with frame f under ITS camera
(tests/gauss_backward_cam_ref.py; tests/test_gauss_backward_cam_ref_cpu.py proves the bars attainable with the float32 C
oracle).

Chain outputs (d_position, d_cubic in both table layouts, d_rotation, d_scaling, d_opacity): per row at geometry_ref's
gradient bar, no outlier budget, onto pre-filled and onto zero buffers, for groups of 1 to 4 frames, a group cut short by a
segment change (the camera follows the frame index, not the lane), 33 frames, the four record layouts; orthographic cameras
per frame, pinhole cameras per frame, and ONE pinhole camera (both strides 0 through CAM = 2).

Linear outputs (feature / set / source gradients with both per-frame-source paths, tap, abs_tap, radii_max): bit for bit, as
the linear tests of the one-camera kernel, over P in {1, 63, 65, 257} x F in {1, 4, 5, 34} and every record stride."""
import numpy as np
import pytest

import gauss_backward_cam_ref as gc
import gauss_backward_ref as gb
import geometry_ref as gr
import test_gpu_gauss_backward_reference as base
import torch_twin as tw

pytestmark = pytest.mark.gpu

SHAPES = [(F, P) for F in gc.LINEAR_F for P in gc.LINEAR_P]
SHAPE_IDS = [f"F{F}-P{P}" for F, P in SHAPES]
LINEAR_MODES = ("pinhole_pf", "ortho_pf", "pinhole_one")


# ------------------------------------------------------------------ chain outputs
def run_chain(gpu, mode, name, lkey):
    Pb = gc.problem(mode, name, lkey)
    c, R, dch, times = Pb["c"], Pb["R"], Pb["depth_channel"], Pb["times"]
    lay, N, I = R["layout"], c["N"], c["I"]
    W, H = c["W"], c["H"]
    layout = tw.SEGMENT_MAJOR if lkey in ("plain_wide", "sets_narrow") else tw.GAUSSIAN_MAJOR
    g = gc.dyn_geometry(mode, c, times, layout, gpu)
    D = gb.upload_records(R, gpu, gb.make_radius(len(times), N))
    pre = base._dyn_grad_prefill(N, I, len(times))
    if (gc.TIMES.index(name) + gc.MODES[mode]["cam"]) % 2 == 0:
        pre = {k: np.zeros_like(v) for k, v in pre.items()}
    o = base._up(pre, gpu)
    if lay["kind"] == "plain":
        gc.call_dynamic_cam(D, g, W, H, o)
    elif lkey == "sets_narrow":
        gc.call_dynamic_sets_cam(D, g, W, H, o, gb.layout_sets_tables(lay, dch), dch)
    else:
        gc.call_dynamic_sources_cam(D, g, W, H, o, [dict(c0=0, cn=3), dict(c0=4, cn=19)], dch)
    got = {k: gb.host(o[k]) for k in gb.DYN_OUT}
    pre_gm = dict(pre)
    for d in (got, pre_gm):
        d["d_cubic"] = gb.cubic_gaussian_major(d["d_cubic"], N, I, layout)
    rep = gr.Report(c)
    gb.check_chain(rep, "", got, Pb["ref"], pre_gm)
    return rep


@pytest.mark.parametrize("lkey", gb.CHAIN_LAYOUTS)
@pytest.mark.parametrize("mode,name", gc.problems(), ids=[f"{m}-{n}" for m, n in gc.problems()])
def test_dynamic_chain_under_cameras_matches_float64(gpu, mode, name, lkey):
    run_chain(gpu, mode, name, lkey).finish()


def test_one_orthographic_camera_is_the_core_entry_point(gpu):
    """perspective == 0 with stride 0 (or F == 1) calls the core twin: the same bits as splat_frames_gauss_backward_dynamic_sets"""
    Pb = gb.dyn_problem("run5", "sets_narrow")
    c, R, dch, times = Pb["c"], Pb["R"], Pb["depth_channel"], Pb["times"]
    W, H = c["W"], c["H"]
    g = gb.dyn_geometry(c, times, tw.GAUSSIAN_MAJOR, gpu)
    g["cam"] = gb.camera_struct(g["extr"])
    D = gb.upload_records(R, gpu, gb.make_radius(len(times), c["N"]))
    pre = base._dyn_grad_prefill(c["N"], c["I"], 3)
    tables = gb.layout_sets_tables(R["layout"], dch)
    a, b = base._up(pre, gpu), base._up(pre, gpu)
    gb.call_dynamic_sets(D, g, W, H, a, tables, dch)
    gc.call_dynamic_sets_cam(D, g, W, H, b, tables, dch)
    for k in pre:
        base._eq(k, gb.host(b[k]), gb.host(a[k]))


# ------------------------------------------------------------------ linear outputs
def _inputs(mode, F, P, layout, gpu):
    c = gc.dyn_case(mode)
    times = [7.0] if F == 1 else [float(t) for t in np.linspace(0.0, 20.0, F)]
    return c, gc.dyn_geometry(mode, c, times, layout, gpu, P)


@pytest.mark.parametrize("F,P", SHAPES, ids=SHAPE_IDS)
def test_linear_outputs_under_cameras(gpu, F, P):
    """_dynamic_cam over every plain stride and _dynamic_sets_cam over every SETS stride, the camera mode rotating"""
    cnt = gb.count_table(F, P)
    radius = gb.make_radius(F, P, 2)
    W, H = gb.W_H
    covered = set()
    for k, (C, want_abs) in enumerate(base.PLAIN_CONFIGS):
        mode = LINEAR_MODES[k % 3]
        lay = gb.plain_layout(C, want_abs)
        covered.add(lay["stride"])
        R = gb.build_records(cnt, lay, seed=40 + k)
        S = gb.segment_sums(R)
        D = gb.upload_records(R, gpu, radius)
        c, g = _inputs(mode, F, P, k % 2, gpu)
        pre = base._dyn_grad_prefill(P, c["I"], k, null=("d_cubic",) if k % 4 == 3 else ())
        if k % 5 != 4:
            pre["d_feature"] = gb.prefill((P, C), k + 9, True)
        base._tap_outputs(pre, P, k, lay)
        o = base._up(pre, gpu)
        gc.call_dynamic_cam(D, g, W, H, o)
        tag = f"{mode} dynamic_cam C{C} abs{want_abs} stride{lay['stride']}: "
        if "d_feature" in pre:
            base._eq(tag + "d_feature", gb.host(o["d_feature"]), base._added(pre["d_feature"], gb.feature_sums(R, S).sum(0), True))
        base._check_taps(o, pre, R, S, W, H, radius, tag)
        none = cnt.sum(0) == 0
        for name in pre:
            if name.startswith("d_") and name not in ("d_feature", "d_cubic"):
                base._eq(tag + name, gb.host(o[name])[none], pre[name][none])
    for k, C in enumerate(base.SETS_CS):
        mode = LINEAR_MODES[(k + 1) % 3]
        lay = gb.sets_layout(C)
        covered.add(lay["stride"])
        R = gb.build_records(cnt, lay, seed=60 + k)
        S = gb.segment_sums(R)
        D = gb.upload_records(R, gpu, radius)
        c, g = _inputs(mode, F, P, (k + 1) % 2, gpu)
        tables, dch, null_set = base._sets_tables(C, k)
        pre = base._dyn_grad_prefill(P, c["I"], k)
        pre.update(base._sets_prefill(P, tables, null_set, k, True))
        base._tap_outputs(pre, P, k, lay)
        o = base._up(pre, gpu)
        gc.call_dynamic_sets_cam(D, g, W, H, o, tables, dch)
        tag = f"{mode} dynamic_sets_cam C{C} stride{lay['stride']} depth{dch}: "
        base._check_sets(o, pre, tables, dch, gb.feature_sums(R, S).sum(0), True, tag)
        base._check_taps(o, pre, R, S, W, H, radius, tag)
    assert sorted(covered) == list(range(8, 41, 4))


@pytest.mark.parametrize("mode", ["ortho_pf", "pinhole_pf"])
@pytest.mark.parametrize("F,P", SHAPES, ids=SHAPE_IDS)
def test_sources_linear_outputs_under_cameras(gpu, F, P, mode):
    """_dynamic_sources_cam: every frame's rows of a per-frame source = that frame's own segment sums (the one-chunk and the
    generic path), the floats between P * cn and the frame stride untouched, the shared source = the sum over the frames"""
    C = 23 if mode == "ortho_pf" else 28
    cnt = gb.count_table(F, P)
    radius = gb.make_radius(F, P, 3)
    W, H = gb.W_H
    lay = gb.sets_layout(C)
    R = gb.build_records(cnt, lay, seed=80 + C)
    S = gb.segment_sums(R)
    D = gb.upload_records(R, gpu, radius)
    feat = gb.feature_sums(R, S)
    dch = 3
    c, g = _inputs(mode, F, P, F % 2, gpu)
    sources = [dict(s, frame_stride=(P * s["cn"] + 7) if s["per_frame"] else 0) for s in base.SOURCES]
    pre = base._dyn_grad_prefill(P, c["I"], 5)
    for n, s in enumerate(sources):
        pre[f"src{n}"] = gb.prefill((F, s["frame_stride"]) if s["frame_stride"] else (P, s["cn"]), 90 + n, True)
    base._tap_outputs(pre, P, 0, lay)
    o = base._up(pre, gpu)
    gc.call_dynamic_sources_cam(D, g, W, H, o, sources, dch)
    for n, s in enumerate(sources):
        c0, cn = s["c0"], s["cn"]
        cols = [x for x in range(cn) if c0 + x != dch]
        rows = [c0 + x for x in cols]
        want = pre[f"src{n}"].copy()
        if s["frame_stride"]:
            body = want[:, :P * cn].reshape(F, P, cn)      # (a view: the gap floats stay the pre-fill)
            body[:, :, cols] = base._added(body[:, :, cols], feat[:, :, rows], True)
        else:
            want[:, cols] = base._added(want[:, cols], feat.sum(0)[:, rows], True)
        base._eq(f"{mode} source{n} ({s['path']}): ", gb.host(o[f"src{n}"]), want)
    base._check_taps(o, pre, R, S, W, H, radius, mode + ": ")
