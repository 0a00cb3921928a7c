"""splat_frames_camera_backward_dynamic (include/splat_hip_camera_grad.h: cam_grad_kernel and its fold) called on its own
with pair records built by the test, against the float64 reference of tests/camera_grad_ref.py at geometry_ref.Report.tensor's
bar (tests/test_camera_grad_ref_cpu.py proves it attainable in float32): every problem -- orthographic cameras per frame,
pinhole cameras per frame, ONE pinhole and ONE orthographic camera (stride 0: the frames' sum), groups of 1 to 4 frames, a
segment change, 33 frames, plain records without and SETS records with a depth column -- and P in {1, 63, 65, 257} (wave and
workgroup tails, more than one partial row per frame), both cubic layouts, ADD onto pre-filled buffers, either output NULL.
Two runs give the same bits, and the sums are finite although the cases hold rows with non-finite positions."""
import numpy as np
import pytest
import torch

import camera_grad_ref as cr
import gauss_backward_ref as gb
import geometry_ref as gr
import torch_twin as tw

pytestmark = pytest.mark.gpu

PROBLEMS = [(m, n, k) for m, n in cr.problems() for k in cr.LAYOUTS]
IDS = [f"{m}-{n}-{k}" for m, n, k in PROBLEMS]


def run(gpu, mode, name, lkey, P=None, layout=tw.GAUSSIAN_MAJOR, prefill=False, want_extr=True, want_intr=True, check=True):
    """one call of the entry point; returns (d_extr, d_intr) as host arrays (None: not asked for)"""
    Pb = cr.problem(mode, name, lkey, P)
    c, R, times = Pb["c"], Pb["R"], Pb["times"]
    F, share, persp = len(times), cr.shared(mode), not cr.MODES[mode]["ortho"]
    g = cr.dyn_geometry(mode, cr.dyn_case(mode), times, layout, gpu, Pb["P"])
    D = gb.upload_records(R, gpu)
    rows = 1 if share else F
    pre_e = gb.prefill((rows, 12), 11, True) if prefill else np.zeros((rows, 12), np.float32)
    pre_i = gb.prefill((rows, 4), 12, True) if prefill else np.zeros((rows, 4), np.float32)
    d_extr = gb.dev(pre_e, gpu) if want_extr else None
    d_intr = gb.dev(pre_i, gpu) if (want_intr and persp) else None
    part = cr.partials(F, Pb["P"], gpu)
    part.fill_(float("nan"))                       # the scratch is written before it is read
    cr.call_camera_backward(D, g, c["W"], c["H"], cr.depth_column(R, Pb["depth_channel"]), part, d_extr, d_intr)
    got_e, got_i = gb.host(d_extr), gb.host(d_intr)
    if check:
        rep = gr.Report(c)
        cr.check(rep, "", got_e, got_i, Pb["ref"], share, pre_e if prefill else None, pre_i if prefill else None)
        rep.finish()
    return got_e, got_i


@pytest.mark.parametrize("mode,name,lkey", PROBLEMS, ids=IDS)
def test_camera_gradients_match_float64(gpu, mode, name, lkey):
    layout = tw.SEGMENT_MAJOR if lkey == "sets_wide" else tw.GAUSSIAN_MAJOR
    got_e, got_i = run(gpu, mode, name, lkey, layout=layout)
    assert np.isfinite(got_e).all() and (got_i is None or np.isfinite(got_i).all())
    if cr.MODES[mode]["ortho"]:      # (the orthographic case's "edge" stratum; tests/test_camera_grad_ref_cpu.py: NaN unmasked)
        assert not np.isfinite(cr.dyn_case(mode)["position"]).all(), "the case holds rows with non-finite positions"


@pytest.mark.parametrize("P", cr.SIZES)
@pytest.mark.parametrize("mode,name", [("ortho_pf", "run5"), ("pinhole_pf", "segments_ABA"), ("pinhole_one", "run5"),
                                       ("ortho_one", "segments_ABA")])
def test_sizes(gpu, mode, name, P):
    run(gpu, mode, name, "sets_wide", P=P, layout=P % 2)


@pytest.mark.parametrize("layout", [tw.GAUSSIAN_MAJOR, tw.SEGMENT_MAJOR])
@pytest.mark.parametrize("mode", ["ortho_pf", "pinhole_pf"])
def test_cubic_layouts(gpu, mode, layout):
    a = run(gpu, mode, "segments_ABA", "plain_narrow", layout=layout)
    b = run(gpu, mode, "segments_ABA", "sets_wide", layout=layout)
    assert not np.array_equal(a[0], b[0])


@pytest.mark.parametrize("mode,name", [("ortho_pf", "run3"), ("pinhole_pf", "run9"), ("pinhole_one", "segments_ABA"),
                                       ("ortho_one", "run5")])
def test_outputs_are_added_to(gpu, mode, name):
    zero = run(gpu, mode, name, "sets_wide")
    pre = run(gpu, mode, name, "sets_wide", prefill=True)
    assert not np.array_equal(zero[0], pre[0])


@pytest.mark.parametrize("mode,name", [("pinhole_pf", "run5"), ("pinhole_one", "run5")])
def test_either_output_may_be_null(gpu, mode, name):
    both = run(gpu, mode, name, "sets_wide")
    e_only = run(gpu, mode, name, "sets_wide", want_intr=False)
    i_only = run(gpu, mode, name, "sets_wide", want_extr=False)
    assert e_only[1] is None and i_only[0] is None
    assert np.array_equal(e_only[0], both[0]) and np.array_equal(i_only[1], both[1])


@pytest.mark.parametrize("mode,name", [("ortho_pf", "frames33"), ("pinhole_pf", "frames33"), ("pinhole_one", "segments_ABA"),
                                       ("ortho_one", "run5")])
def test_two_runs_give_the_same_bits(gpu, mode, name):
    a = run(gpu, mode, name, "sets_wide", prefill=True, check=False)
    b = run(gpu, mode, name, "sets_wide", prefill=True, check=False)
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(x.view(np.int32), y.view(np.int32))


def test_orthographic_camera_takes_no_intrinsics_gradient(gpu):
    Pb = cr.problem("ortho_pf", "run2", "plain_narrow")
    c, R = Pb["c"], Pb["R"]
    g = cr.dyn_geometry("ortho_pf", cr.dyn_case("ortho_pf"), Pb["times"], tw.GAUSSIAN_MAJOR, gpu)
    D = gb.upload_records(R, gpu)
    buf = torch.zeros(2, 12, device=gpu)
    L = gb.lib()
    with pytest.raises(L.SplatError, match="d_intr belongs to the perspective camera"):
        cr.call_camera_backward(D, g, c["W"], c["H"], -1, cr.partials(2, R["P"], gpu), buf, torch.zeros(2, 4, device=gpu))
    assert not buf.any()
