"""The test of the dynamic batch's Gaussian-side backward under per-frame and pinhole cameras
(tests/test_gpu_gauss_backward_dynamic_cam.py) proven on the CPU before any kernel runs: which rows receive records under
every frame's camera, and the float32 C oracle's chain per frame -- its dynamic evaluation, its operators under the frame's
camera, its dynamic backward, summed -- inside the bars the HIP kernel is held to, on every row of the same problems
(tests/gauss_backward_cam_ref.py)."""
import numpy as np
import pytest

import gauss_backward_cam_ref as gc
import gauss_backward_ref as gb
import geometry_ref as gr


@pytest.mark.parametrize("mode,name", gc.problems(), ids=[f"{m}-{n}" for m, n in gc.problems()])
def test_rows_that_receive_records(mode, name):
    e = gc.eligibility(mode, name)
    times = gb.DYN_TIMES[name]
    assert e.shape == (len(times), gc.dyn_case(mode)["N"])
    assert e.any(0).mean() >= 0.25
    assert e[:, list(gb.DYN_HARD_ROWS)].any(0).all(), "every hard row owns a record in at least one frame"
    P = gc.problem(mode, name, "plain_narrow")
    assert (P["R"]["cnt"][:, list(gb.DYN_HARD_ROWS)].sum(0) > 0).all()
    assert (P["R"]["cnt"][~e] == 0).all(), "records go only to rows eligible in that frame under that frame's camera"
    segs = gb.segments(gc.dyn_case(mode), times)
    if name == "segments_ABA":       # groups cut short by the segment change: 2 + 3 + 2 frames, cameras 0 1 | 2 3 4 | 5 6
        assert segs[0] == segs[-1] != segs[2] and len(set(segs)) == 2
    if name.startswith("run"):
        assert len(set(segs)) == 1 and len(segs) == int(name[3:])
    if name == "frames33":
        assert len(times) > 32 and (e[16:].mean(1) > 0).all(), "the late frames' cameras still see rows"


def test_cameras_differ_per_frame():
    c = gc.dyn_case("pinhole_pf")
    k0, e0 = gc.frame_camera("pinhole_pf", c, 0)
    k3, e3 = gc.frame_camera("pinhole_pf", c, 3)
    assert not np.array_equal(k0, k3) and not np.array_equal(e0, e3)
    assert np.array_equal(k0, c["intr"]) and np.array_equal(e0, c["extr"])       # frame 0 = the case's own camera
    k, e = gc.frame_camera("pinhole_one", c, 3)
    assert k is c["intr"] and e is c["extr"]
    o = gc.dyn_case("ortho_pf")
    assert not np.array_equal(gc.frame_camera("ortho_pf", o, 1)[1], gc.frame_camera("ortho_pf", o, 2)[1])
    assert not c["ortho"] and o["ortho"]


@pytest.mark.parametrize("lkey", ["plain_narrow", "sets_wide"])
@pytest.mark.parametrize("mode,name", gc.problems(), ids=[f"{m}-{n}" for m, n in gc.problems()])
def test_oracle_chain_meets_the_bars(oracle_mod, mode, name, lkey):
    P = gc.problem(mode, name, lkey)
    rep = gr.Report(P["c"])
    got = gc.oracle_dynamic(oracle_mod, mode, gc.dyn_case(mode), P["times"], P["R"], P["S"], P["depth_channel"])
    gb.check_chain(rep, "", got, P["ref"])
    rep.finish()
