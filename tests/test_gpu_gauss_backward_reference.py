"""The frame batch's Gaussian-side backward kernels (frames_gauss_bwd_static_kernel, frames_gauss_bwd_dynamic_kernel and
splat_pair_records_segment_sum, csrc/preprocess.hip) called on their own with pair records built by the test -- the
compositor is not involved -- against float64 (tests/gauss_backward_ref.py; tests/test_gauss_backward_ref_cpu.py proves the
bars attainable with the float32 C oracle).

Linear outputs (feature / set / source gradients, the static kernels' d_opacity, tap, abs_tap, radii_max, the segment sum):
bit for bit against the float64 sums -- the record values make every float32 sum exact in any order -- over the full grid
P in {1, 63, 64, 65, 257} x F in {1, 2, 3, 4, 5, 33, 34}: frames past the 32 whose slot ranges the static kernel keeps in
LDS, record counts on both sides of every request width (6 and 12 narrow, 2 and 6 wide), P on both sides of a workgroup's 64
Gaussians, every record stride the library hands out, the three camera modes, accumulate / skip_opacity / depth_channel /
NULL outputs, SETS and SOURCES routing with both per-frame-source paths.  Unowned slots and padding floats are NaN.

Chain outputs (d_xyz, d_scales, d_uquats; d_position, d_cubic in both table layouts, d_rotation, d_scaling, d_opacity):
per row against the float64 twin's chain at geometry_ref's gradient bar, no outlier budget, on the hard geometry cases
o257 / p257 and the dynamic case's quaternion sums of norm 1e-10 .. 0 and opacity logits +-30."""
import numpy as np
import pytest
import torch

import gauss_backward_ref as gb
import geometry_ref as gr
import torch_twin as tw

pytestmark = pytest.mark.gpu

# (C, want_abs) of the plain records: every stride splat_blend_pair_stride hands out (8 12 16 24 28 32 40), widths that fill
# their chunk and widths that leave padding channels inside it
PLAIN_CONFIGS = [(1, 0), (2, 0), (3, 1), (5, 1), (8, 0), (16, 1), (17, 0), (24, 1), (32, 0), (32, 1)]
# row widths of the SETS records: strides 16 .. 40; 23 = the renderer's plan
SETS_CS = [2, 4, 5, 12, 13, 17, 23, 28]
SHAPES = [(F, P) for F in gb.LINEAR_F for P in gb.LINEAR_P]
SHAPE_IDS = [f"F{F}{'_past_lds' if F > 32 else ''}-P{P}" for F, P in SHAPES]
GRAD_NAMES = ("d_xyz", "d_scales", "d_uquats")


def _eq(name, got, want):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want), err_msg=name)


def _up(pre, gpu):
    return {k: gb.dev(v, gpu) for k, v in pre.items()}


def _static_inputs(F, P, cam, gpu):
    c, frames = gb.static_frames(gb.CHAIN_CAMS[cam], F, cam)
    return c, frames, gb.static_geometry(c, frames, cam, gpu, P)


def _tap_outputs(pre, P, k, lay):
    """tap / abs_tap / radii_max each given or NULL, rotating with k"""
    if k % 2 == 0:
        pre["tap"] = np.full((P, 2), np.nan, np.float32)
    if lay["abs"] is not None and k % 3 != 1:
        pre["abs_tap"] = np.full((P, 2), np.nan, np.float32)
    if k % 4 != 3:
        pre["radii_max"] = np.full(P, -7, np.int32)


def _check_taps(o, pre, R, S, W, H, radius, tag):
    lay = R["layout"]
    if "tap" in pre:
        _eq(tag + "tap", gb.host(o["tap"]), gb.taps(R, S, W, H, lay["tap"]))
    if "abs_tap" in pre:
        _eq(tag + "abs_tap", gb.host(o["abs_tap"]), gb.taps(R, S, W, H, lay["abs"]))
    if "radii_max" in pre:
        _eq(tag + "radii_max", gb.host(o["radii_max"]), radius.max(0))


def _added(pre, total, accumulate):
    """what a kernel leaves where it stores / adds ``total`` (float64, exact)"""
    return (pre.astype(np.float64) + total).astype(np.float32) if accumulate else total.astype(np.float32)


def _geometry_prefill(P, k, acc):
    return dict(d_xyz=gb.prefill((P, 3), k, acc), d_scales=gb.prefill((P, 3), k + 1, acc), d_uquats=gb.prefill((P, 4), k + 2, acc),
                d_opacity=gb.prefill((P, 1), k + 3, acc))


# ------------------------------------------------------------------ linear outputs, static kernels
@pytest.mark.parametrize("F,P", SHAPES, ids=SHAPE_IDS)
def test_static_plain_linear_outputs(gpu, F, P):
    """splat_frames_gauss_backward_static / _set / _cam over every plain stride and the three camera modes"""
    cnt = gb.count_table(F, P)
    radius = gb.make_radius(F, P)
    W, H = gb.W_H
    covered = set()
    for k, (C, want_abs) in enumerate(PLAIN_CONFIGS):
        lay = gb.plain_layout(C, want_abs)
        covered.add(lay["stride"])
        R = gb.build_records(cnt, lay, seed=k)
        S = gb.segment_sums(R)
        D = gb.upload_records(R, gpu, radius)
        feat = gb.feature_sums(R, S).sum(0)
        for cam in (0, 1, 2):
            c, frames, g = _static_inputs(F, P, cam, gpu)
            m = k + cam
            entry = ("static", "set", "cam")[k % 3] if cam == 0 else "cam"
            acc = m % 2
            plainest = entry == "static"
            skip = 0 if plainest else (k // 2 + cam) % 2
            dch = -1 if (plainest or k % 2 == 0) else (C - 1) // 2
            fs = C if plainest else C + k % 3
            pre = _geometry_prefill(P, m, acc)
            if plainest or k % 5 != 4:
                pre["d_feature"] = gb.prefill((P, fs), m + 4, acc)
            _tap_outputs(pre, P, m, lay)
            o = _up(pre, gpu)
            tag = f"C{C} abs{want_abs} stride{lay['stride']} cam{cam} {entry} acc{acc} skip{skip} depth{dch}: "
            if entry == "static":
                gb.call_static(D, g, W, H, o, acc)
            elif entry == "set":
                gb.call_static_set(D, g, W, H, o, acc, fs, skip, dch)
            else:
                gb.call_static_cam(D, g, W, H, o, g["cam"], acc, fs, skip, dch)
            want = pre["d_opacity"] if skip else _added(pre["d_opacity"], S[:, :, 5].sum(0)[:, None], acc)
            _eq(tag + "d_opacity", gb.host(o["d_opacity"]), want)
            if "d_feature" in pre:
                want = pre["d_feature"].copy()
                ch = [x for x in range(C) if x != dch]
                want[:, ch] = _added(pre["d_feature"][:, ch], feat[:, ch], acc)
                _eq(tag + "d_feature", gb.host(o["d_feature"]), want)
                assert np.isfinite(want[:, ch]).all()
            _check_taps(o, pre, R, S, W, H, radius, tag)
            if acc:   # rows without any record keep the pre-fill of the chain outputs bit for bit
                none = cnt.sum(0) == 0
                for name in GRAD_NAMES:
                    _eq(tag + name, gb.host(o[name])[none], pre[name][none])
    assert sorted(covered) == gb.plain_strides()


def _sets_tables(C, k):
    """three sets that tile the row (the renderer's plan at C = 23), the depth channel, and which set pointers are NULL"""
    if C == gb.PLAN23["C"]:
        c0, cn, dch = gb.PLAN23["c0"], gb.PLAN23["cn"], gb.PLAN23["depth_channel"]
    else:
        a = min(3, C - 1)
        b = 1 if C - a > 1 else 0
        c0, cn = (0, a, a + b), (a, b, C - a - b)
        dch = a if (b and k % 2 == 0) else -1
    stride = tuple(max(n, 1) + (k + g_) % 2 for g_, n in enumerate(cn))
    return dict(c0=c0, cn=cn, stride=stride), dch, k % 3       # the set (k % 3) gets a NULL pointer


def _sets_prefill(P, tables, null_set, seed, acc):
    return {f"set{g_}": gb.prefill((P, tables["stride"][g_]), seed + g_, acc)
            for g_ in range(3) if tables["cn"][g_] > 0 and g_ != null_set}


def _check_sets(o, pre, tables, dch, feat, acc, tag):
    for g_ in range(3):
        if f"set{g_}" not in pre:
            continue
        c0, cn = tables["c0"][g_], tables["cn"][g_]
        want = pre[f"set{g_}"].copy()
        cols = [x for x in range(cn) if c0 + x != dch]
        rows = [c0 + x for x in cols]
        want[:, cols] = _added(want[:, cols], feat[:, rows], acc)
        _eq(tag + f"set{g_}", gb.host(o[f"set{g_}"]), want)
        assert np.isfinite(want[:, cols]).all()


@pytest.mark.parametrize("F,P", SHAPES, ids=SHAPE_IDS)
def test_static_sets_linear_outputs(gpu, F, P):
    """splat_frames_gauss_backward_static_sets / _sets_cam / _sources_cam over every SETS stride and the three camera modes"""
    cnt = gb.count_table(F, P)
    radius = gb.make_radius(F, P, 1)
    W, H = gb.W_H
    covered = set()
    for k, C in enumerate(SETS_CS):
        lay = gb.sets_layout(C)
        covered.add(lay["stride"])
        R = gb.build_records(cnt, lay, seed=20 + k)
        S = gb.segment_sums(R)
        D = gb.upload_records(R, gpu, radius)
        feat = gb.feature_sums(R, S).sum(0)
        for cam in (0, 1, 2):
            c, frames, g = _static_inputs(F, P, cam, gpu)
            m = k + cam
            acc = m % 2
            tables, dch, null_set = _sets_tables(C, m)
            pre = _geometry_prefill(P, m, acc)
            _tap_outputs(pre, P, m, lay)
            tag = f"C{C} stride{lay['stride']} cam{cam} acc{acc} depth{dch}: "
            if k % 3 == 2:      # the same routing as a SOURCES table (shared sources; one of them without a gradient)
                sources = [dict(c0=tables["c0"][g_], cn=tables["cn"][g_]) for g_ in range(3) if tables["cn"][g_] > 0]
                keep = [g_ for g_ in range(3) if tables["cn"][g_] > 0]
                for n, g_ in enumerate(keep):
                    if g_ != null_set:
                        pre[f"src{n}"] = gb.prefill((P, tables["cn"][g_]), m + g_, acc)
                o = _up(pre, gpu)
                gb.call_static_sources_cam(D, g, W, H, o, g["cam"], sources, acc, dch)
                for n, g_ in enumerate(keep):
                    if f"src{n}" in pre:
                        c0, cn = tables["c0"][g_], tables["cn"][g_]
                        want = pre[f"src{n}"].copy()
                        cols = [x for x in range(cn) if c0 + x != dch]
                        want[:, cols] = _added(want[:, cols], feat[:, [c0 + x for x in cols]], acc)
                        _eq(tag + f"source{n}", gb.host(o[f"src{n}"]), want)
            else:
                pre.update(_sets_prefill(P, tables, null_set, m, acc))
                o = _up(pre, gpu)
                if cam == 0 and k % 2 == 0:
                    gb.call_static_sets(D, g, W, H, o, tables, acc, dch)
                else:
                    gb.call_static_sets_cam(D, g, W, H, o, g["cam"], tables, acc, dch)
                _check_sets(o, pre, tables, dch, feat, acc, tag)
            _eq(tag + "d_opacity", gb.host(o["d_opacity"]), _added(pre["d_opacity"], S[:, :, 5].sum(0)[:, None], acc))
            _check_taps(o, pre, R, S, W, H, radius, tag)
    assert sorted(covered) == gb.sets_strides()


# ------------------------------------------------------------------ linear outputs, dynamic kernels
def _dyn_inputs(F, P, layout, gpu):
    c = gb.dyn_case()
    times = [7.0] if F == 1 else [float(t) for t in np.linspace(0.0, 20.0, F)]
    return c, times, gb.dyn_geometry(c, times, layout, gpu, P)


def _dyn_grad_prefill(P, I, seed, null=()):
    shapes = dict(d_position=(P, 3), d_cubic=(P * 4 * I * 3,), d_rotation=(P, 4), d_opacity=(P, 1), d_scaling=(P, 3))
    return {k: gb.prefill(s, seed + n, True) for n, (k, s) in enumerate(shapes.items()) if k not in null}


@pytest.mark.parametrize("F,P", SHAPES, ids=SHAPE_IDS)
def test_dynamic_linear_outputs(gpu, F, P):
    """splat_frames_gauss_backward_dynamic (every plain stride) and _dynamic_sets (every SETS stride): narrow records six at
    a time, wide records two at a time and a last odd one"""
    cnt = gb.count_table(F, P)
    radius = gb.make_radius(F, P, 2)
    W, H = gb.W_H
    for k, (C, want_abs) in enumerate(PLAIN_CONFIGS):
        lay = gb.plain_layout(C, want_abs)
        R = gb.build_records(cnt, lay, seed=40 + k)
        S = gb.segment_sums(R)
        D = gb.upload_records(R, gpu, radius)
        c, times, g = _dyn_inputs(F, P, k % 2, gpu)
        pre = _dyn_grad_prefill(P, c["I"], k, null=("d_cubic",) if k % 4 == 3 else ())
        if k % 5 != 4:
            pre["d_feature"] = gb.prefill((P, C), k + 9, True)
        _tap_outputs(pre, P, k, lay)
        o = _up(pre, gpu)
        gb.call_dynamic(D, g, W, H, o)
        tag = f"dynamic C{C} abs{want_abs} stride{lay['stride']}: "
        if "d_feature" in pre:
            _eq(tag + "d_feature", gb.host(o["d_feature"]), _added(pre["d_feature"], gb.feature_sums(R, S).sum(0), True))
        _check_taps(o, pre, R, S, W, H, radius, tag)
        none = cnt.sum(0) == 0
        for name in pre:
            if name.startswith("d_") and name not in ("d_feature", "d_cubic"):
                _eq(tag + name, gb.host(o[name])[none], pre[name][none])
    for k, C in enumerate(SETS_CS):
        lay = gb.sets_layout(C)
        R = gb.build_records(cnt, lay, seed=60 + k)
        S = gb.segment_sums(R)
        D = gb.upload_records(R, gpu, radius)
        c, times, g = _dyn_inputs(F, P, (k + 1) % 2, gpu)
        tables, dch, null_set = _sets_tables(C, k)
        pre = _dyn_grad_prefill(P, c["I"], k)
        pre.update(_sets_prefill(P, tables, null_set, k, True))
        _tap_outputs(pre, P, k, lay)
        o = _up(pre, gpu)
        gb.call_dynamic_sets(D, g, W, H, o, tables, dch)
        tag = f"dynamic_sets C{C} stride{lay['stride']} depth{dch}: "
        _check_sets(o, pre, tables, dch, gb.feature_sums(R, S).sum(0), True, tag)
        _check_taps(o, pre, R, S, W, H, radius, tag)


# per-frame sources of the dynamic kernel: inside one 16-byte chunk (the one-chunk fast path, spfq >= 0, at element 1 of its
# chunk), chunk-aligned (fast path), and three channels from (12 + c0) % 4 == 3 that straddle a chunk boundary (generic path);
# plus a shared source, which receives the sum over the frames
SOURCES = [dict(c0=1, cn=2, per_frame=True, path="one_chunk"), dict(c0=4, cn=4, per_frame=True, path="one_chunk_aligned"),
           dict(c0=11, cn=3, per_frame=True, path="generic_straddling"), dict(c0=14, cn=6, per_frame=False, path="shared")]


@pytest.mark.parametrize("C", [23, 28])
@pytest.mark.parametrize("F,P", SHAPES, ids=SHAPE_IDS)
def test_dynamic_sources_linear_outputs(gpu, F, P, C):
    """splat_frames_gauss_backward_dynamic_sources: every frame's rows of a per-frame source = that frame's own segment sums
    (both paths), the floats between P * cn and the frame stride untouched, the shared source = the sum over the frames"""
    assert [(gb.SETS_NG + s["c0"]) // 4 == (gb.SETS_NG + s["c0"] + s["cn"] - 1) // 4 for s in SOURCES[:3]] == [True, True, False]
    assert (gb.SETS_NG + SOURCES[2]["c0"]) % 4 == 3
    cnt = gb.count_table(F, P)
    radius = gb.make_radius(F, P, 3)
    W, H = gb.W_H
    lay = gb.sets_layout(C)
    R = gb.build_records(cnt, lay, seed=80 + C)
    S = gb.segment_sums(R)
    D = gb.upload_records(R, gpu, radius)
    feat = gb.feature_sums(R, S)
    dch = 3
    for variant in ("per_frame_and_shared", "shared_only"):
        c, times, g = _dyn_inputs(F, P, F % 2, gpu)
        sources = [dict(s, frame_stride=(P * s["cn"] + 7) if s["per_frame"] else 0) for s in SOURCES]
        if variant == "shared_only":
            sources = [dict(c0=0, cn=4, frame_stride=0), dict(c0=4, cn=C - 4, frame_stride=0)]
        pre = _dyn_grad_prefill(P, c["I"], 5)
        for n, s in enumerate(sources):
            pre[f"src{n}"] = gb.prefill((F, s["frame_stride"]) if s["frame_stride"] else (P, s["cn"]), 90 + n, True)
        _tap_outputs(pre, P, 0, lay)
        o = _up(pre, gpu)
        gb.call_dynamic_sources(D, g, W, H, o, sources, dch)
        for n, s in enumerate(sources):
            c0, cn = s["c0"], s["cn"]
            cols = [x for x in range(cn) if c0 + x != dch]
            rows = [c0 + x for x in cols]
            want = pre[f"src{n}"].copy()
            if s["frame_stride"]:
                body = want[:, :P * cn].reshape(F, P, cn)      # (a view: the gap floats stay the pre-fill)
                body[:, :, cols] = _added(body[:, :, cols], feat[:, :, rows], True)
            else:
                want[:, cols] = _added(want[:, cols], feat.sum(0)[:, rows], True)
            _eq(f"{variant} source{n} ({s.get('path', 'shared')}): ", gb.host(o[f"src{n}"]), want)
        _check_taps(o, pre, R, S, W, H, radius, variant + ": ")


@pytest.mark.parametrize("F,P", SHAPES, ids=SHAPE_IDS)
def test_segment_sum(gpu, F, P):
    """splat_pair_records_segment_sum at every record stride, on the first and the last frame of the record set"""
    cnt = gb.count_table(F, P)
    for k, lay in enumerate([gb.plain_layout(C, a) for C, a in PLAIN_CONFIGS] + [gb.sets_layout(C) for C in SETS_CS]):
        R = gb.build_records(cnt, lay, seed=100 + k)
        S = gb.segment_sums(R)
        D = gb.upload_records(R, gpu)
        for f in sorted({0, F - 1}):
            out = gb.dev(np.full((P, lay["stride"]), np.nan, np.float32), gpu)
            gb.call_segment_sum(D, f, out)
            _eq(f"{lay['kind']} stride {lay['stride']} frame {f}: ", gb.host(out)[:, lay["used"]],
                S[f][:, lay["used"]].astype(np.float32))


def test_wide_range_sums(gpu):
    """records of log-uniform size 1e-6 .. 1e3 and random sign: every linear sum within the a priori bound of a float32 sum
    of n terms in any order, (n - 1) 2^-24 sum|v|  (the taps, which add a product's rounding, are not taken)"""
    F, P = 5, 257
    W, H = gb.W_H
    cnt = gb.count_table(F, P)
    lay = gb.plain_layout(8, True)
    R = gb.build_records(cnt, lay, seed=7, wide_range=True)
    S, A = gb.segment_sums(R), gb.segment_sums(R, absolute=True)
    D = gb.upload_records(R, gpu)
    n = cnt.sum(0)[:, None]

    def inside(name, got, ref, mag, terms):
        err = np.abs(got.astype(np.float64) - ref)
        bound = np.maximum(terms - 1, 0) * gr.EPS32 * mag
        assert np.isfinite(got).all() and (err <= bound).all(), f"{name}: {float((err / np.maximum(bound, 1e-300)).max()):.3g}x the bound"

    ng, C = lay["ng"], lay["C"]
    for cam in (0, 1, 2):
        c, frames, g = _static_inputs(F, P, cam, gpu)
        pre = _geometry_prefill(P, 0, 0)
        pre["d_feature"] = gb.prefill((P, C), 0, 0)
        o = _up(pre, gpu)
        gb.call_static_cam(D, g, W, H, o, g["cam"])
        inside(f"cam{cam} d_feature", gb.host(o["d_feature"]), S.sum(0)[:, ng:ng + C], A.sum(0)[:, ng:ng + C], n)
        inside(f"cam{cam} d_opacity", gb.host(o["d_opacity"]), S.sum(0)[:, 5:6], A.sum(0)[:, 5:6], n)
    c, times, g = _dyn_inputs(F, P, 1, gpu)
    pre = {k: np.zeros_like(v) for k, v in _dyn_grad_prefill(P, c["I"], 0).items()}
    pre["d_feature"] = np.zeros((P, C), np.float32)
    o = _up(pre, gpu)
    gb.call_dynamic(D, g, W, H, o)
    inside("dynamic d_feature", gb.host(o["d_feature"]), S.sum(0)[:, ng:ng + C], A.sum(0)[:, ng:ng + C], n)
    out = gb.dev(np.full((P, lay["stride"]), np.nan, np.float32), gpu)
    gb.call_segment_sum(D, F - 1, out)
    inside("segment sum", gb.host(out)[:, lay["used"]], S[F - 1][:, lay["used"]], A[F - 1][:, lay["used"]], cnt[F - 1][:, None])


# ------------------------------------------------------------------ chain outputs
def run_static_chain(gpu, F, cam, lkey):
    """one static chain problem through the kernel -> (Report, problem, outputs, pre-fill)"""
    Pb = gb.static_problem(F, cam, lkey)
    c, R, dch = Pb["c"], Pb["R"], Pb["depth_channel"]
    lay, N = R["layout"], Pb["c"]["N"]
    W, H = c["W"], c["H"]
    acc = 1 if F in (3, 34) else 0
    g = gb.static_geometry(c, Pb["frames"], cam, gpu)
    D = gb.upload_records(R, gpu, gb.make_radius(F, N))
    pre = _geometry_prefill(N, F + cam, acc)
    if lkey == "plain_narrow":
        pre["d_feature"] = gb.prefill((N, lay["C"]), 1, acc)
        o = _up(pre, gpu)
        if cam == 0:
            gb.call_static(D, g, W, H, o, acc)
        else:
            gb.call_static_cam(D, g, W, H, o, g["cam"], acc)
    elif lkey == "plain_wide":
        o = _up(pre, gpu)
        if cam == 0:
            gb.call_static_set(D, g, W, H, o, acc, None, 0, dch)
        else:
            gb.call_static_cam(D, g, W, H, o, g["cam"], acc, None, 0, dch)
    elif lkey == "sets_narrow":
        tables = gb.layout_sets_tables(lay, dch)
        o = _up(pre, gpu)
        if cam == 0:
            gb.call_static_sets(D, g, W, H, o, tables, acc, dch)
        else:
            gb.call_static_sets_cam(D, g, W, H, o, g["cam"], tables, acc, dch)
    else:
        o = _up(pre, gpu)
        gb.call_static_sources_cam(D, g, W, H, o, g["cam"], [dict(c0=0, cn=3), dict(c0=4, cn=19)], acc, dch)
    rep = gr.Report(c)
    got = {k: gb.host(o[k]) for k in GRAD_NAMES}
    gb.check_chain(rep, "", got, Pb["ref"], pre if acc else None)
    _eq("d_opacity", gb.host(o["d_opacity"]), _added(pre["d_opacity"], Pb["S"][:, :, 5].sum(0)[:, None], acc))
    return rep


@pytest.mark.parametrize("lkey", gb.CHAIN_LAYOUTS)
@pytest.mark.parametrize("cam", [0, 1, 2], ids=["one_ortho_camera", "ortho_camera_per_frame", "pinhole_per_frame"])
@pytest.mark.parametrize("F", gb.CHAIN_F)
def test_static_chain_matches_float64(gpu, F, cam, lkey):
    run_static_chain(gpu, F, cam, lkey).finish()


def run_dyn_chain(gpu, name, lkey):
    Pb = gb.dyn_problem(name, lkey)
    c, R, dch, times = Pb["c"], Pb["R"], Pb["depth_channel"], Pb["times"]
    lay, N, I = R["layout"], c["N"], c["I"]
    W, H = c["W"], c["H"]
    layout = tw.SEGMENT_MAJOR if lkey in ("plain_wide", "sets_narrow") else tw.GAUSSIAN_MAJOR
    g = gb.dyn_geometry(c, times, layout, gpu)
    D = gb.upload_records(R, gpu, gb.make_radius(len(times), N))
    pre = _dyn_grad_prefill(N, I, len(times))
    if sorted(gb.DYN_TIMES).index(name) % 2 == 0:
        pre = {k: np.zeros_like(v) for k, v in pre.items()}
    o = _up(pre, gpu)
    if lay["kind"] == "plain":
        gb.call_dynamic(D, g, W, H, o)
    elif lkey == "sets_narrow":
        gb.call_dynamic_sets(D, g, W, H, o, gb.layout_sets_tables(lay, dch), dch)
    else:
        gb.call_dynamic_sources(D, g, W, H, o, [dict(c0=0, cn=3), dict(c0=4, cn=19)], dch)
    got = {k: gb.host(o[k]) for k in gb.DYN_OUT}
    pre_gm = dict(pre)
    for d in (got, pre_gm):
        d["d_cubic"] = gb.cubic_gaussian_major(d["d_cubic"], N, I, layout)
    rep = gr.Report(c)
    gb.check_chain(rep, "", got, Pb["ref"], pre_gm)
    return rep


@pytest.mark.parametrize("lkey", gb.CHAIN_LAYOUTS)
@pytest.mark.parametrize("name", sorted(gb.DYN_TIMES))
def test_dynamic_chain_matches_float64(gpu, name, lkey):
    """frame groups of up to four of one segment, the flush of d_cubic when the segment changes and when it comes back
    (segments_ABA), the first and last frame and every knot, 33 frames"""
    run_dyn_chain(gpu, name, lkey).finish()
