"""The per-Gaussian geometry of the HIP path against the float64 twin (tests/torch_twin.py) on the hard cases of
tests/geometry_ref.py: rotated and translated cameras, fx != fy with an off-centre principal point, sizes from 0.05 px to
thousands of pixels, isotropic and near-isotropic scales, quaternions of norm 1/2 .. 2, thin splats, rows placed on both
sides of every cull bound, behind the camera, at tz == 0 and at non-finite positions.  Every row is compared on its own
(no outlier budget, no tensor-wide maximum); a row leaves one comparison only when float64 says it sits on that decision,
and its bar widens only with its float64 conditioning.  The bars and margins are those of geometry_ref.py, which
tests/test_geometry_ref_cpu.py proves attainable with the float32 C oracle.

Covered: the individual operators, the fused preprocess operators forward and backward (offset, gradient sinks), the
dynamic evaluation, and the per-Gaussian buffers FrameBatch fills in its forward pass.  The batch's Gaussian-side BACKWARD
reads per-pair records from the compositor: tests/test_gpu_gauss_backward_reference.py calls those kernels on their own,
with records built by the test, against the same float64 twin and bars."""
import numpy as np
import pytest
import torch

import geometry_ref as gr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", gr.CASE_IDS)
def test_operators_match_float64(gpu, cid):
    """gs.project_point / project_point_ortho, compute_cov3d, ewa_project / ewa_project_ortho, values and gradients
    (dL/dintr and dL/dextr on the pinhole path)"""
    c = gr.case_by_id(cid)
    rep = gr.Report(c)
    gr.run_operators(gr.HipBackend(gpu), c, rep)
    rep.finish()


@pytest.mark.parametrize("sink", [False, True])
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("cid", gr.CASE_IDS)
def test_fused_preprocess_matches_float64(gpu, cid, offset, sink):
    """gs.preprocess_ortho / gs.preprocess_persp forward and backward, with and without ``offset`` and gradient sinks"""
    c = gr.case_by_id(cid)
    rep = gr.Report(c)
    gr.run_fused(gr.HipBackend(gpu, sink=sink), c, rep, offset)
    rep.finish()


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_matches_float64(gpu, deg, free):
    c = gr.make_sh_case(deg)
    rep = gr.Report(c)
    gr.run_sh(gr.HipBackend(gpu), c, rep, free)
    rep.finish()


@pytest.mark.parametrize("layout", [0, 1], ids=["gaussian_major", "segment_major"])
@pytest.mark.parametrize("N", gr.DYN_SIZES)
def test_dynamic_evaluate_matches_float64(gpu, N, layout):
    """dynamics.evaluate in both spline-table layouts: first and last frame, every knot, frames inside segments;
    quaternion sums of norm 1e-10 .. 0, opacity logits +-30, scaling logits -12 .. +3"""
    c = gr.make_dyn_case(N)
    rep = gr.Report(c)
    for t in c["times"]:
        gr.run_dyn(gr.HipBackend(gpu), c, rep, t, layout)
    rep.finish()


@pytest.mark.parametrize("N", gr.DYN_SIZES)
def test_position_poly_fourier_matches_float64(gpu, N):
    c = gr.make_dyn_case(N)
    rep = gr.Report(c)
    for t in c["times"]:
        gr.run_ppf(gr.HipBackend(gpu), c, rep, t)
    rep.finish()


@pytest.mark.parametrize("layout", [0, 1], ids=["gaussian_major", "segment_major"])
@pytest.mark.parametrize("cid", ["o257", "o100003"])
def test_frame_preprocess_matches_float64(gpu, cid, layout):
    """dynamics.frame_preprocess (dynamic evaluation fused with the orthographic preprocess), forward and backward"""
    c = gr.make_dyn_geom_case(cid)
    rep = gr.Report(c)
    for t in (0, c["times"][2], c["T"] - 1):
        gr.run_frame_preprocess(gr.HipBackend(gpu), c, rep, t, layout)
    rep.finish()


# ------------------------------------------------------------------ FrameBatch, forward only
def _dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), device=gpu)


def _batch_buffers(fb, f):
    n = lambda x: x[f].cpu().numpy()
    return dict(uv=n(fb.uv), depth=n(fb.depth), conic=n(fb.conic), radius=n(fb.radius))


@pytest.mark.parametrize("cid", ["o257", "p257", "o3001", "p3001"])
def test_frame_batch_buffers_match_float64(gpu, cid):
    """the uv / depth / conic / radius buffers FrameBatch.render fills: one orthographic camera per frame, and the pinhole
    camera with per-frame extrinsics, intrinsics and offsets"""
    from splatter_a_video_amd.frames import FrameBatch
    c = gr.case_by_id(cid)
    F, N = 3, c["N"]
    frames = gr.frame_cases(c, F, offsets=not c["ortho"])
    rng = np.random.default_rng(5)
    opacity = _dev(rng.uniform(0.1, 0.9, size=(N, 1)).astype(np.float32), gpu)
    feature = _dev(rng.uniform(size=(N, 3)).astype(np.float32), gpu)
    xyz = c["xyz"]
    fb = FrameBatch(F, N, c["W"], c["H"], 3, gpu)
    extr = _dev(np.stack([fc["extr"] for fc in frames]), gpu)
    with torch.no_grad():
        if c["ortho"]:
            fb.render(_dev(xyz, gpu), _dev(c["scale"], gpu), _dev(c["quat"], gpu), opacity, feature, None, extr,
                      nearest=c["nearest"], extent=c["extent"])
        else:
            fb.render(_dev(xyz, gpu), _dev(c["scale"], gpu), _dev(c["quat"], gpu), opacity, feature,
                      _dev(np.stack([fc["offset"] for fc in frames]), gpu), extr, nearest=c["nearest"], extent=c["extent"],
                      intr=_dev(np.stack([fc["intr"] for fc in frames]), gpu))
    torch.cuda.synchronize()
    fb.check()
    rep = gr.Report(c)
    for f, fc in enumerate(frames):
        gr.check_chain(rep, f"batch.f{f}.", gr.chain_ref(fc, offset=not c["ortho"]), _batch_buffers(fb, f))
    rep.finish()


@pytest.mark.parametrize("cid", ["o257", "o3001"])
def test_frame_batch_dynamic_buffers_match_float64(gpu, cid):
    """the same buffers after FrameBatch.render_dynamic (dynamic evaluation inside the batched preprocess)"""
    from splatter_a_video_amd import dynamics as dy
    from splatter_a_video_amd.frames import FrameBatch
    c = gr.make_dyn_geom_case(cid)
    N, I = c["N"], c["I"]
    times = [0, c["times"][2], c["T"] - 1]
    rng = np.random.default_rng(6)
    feature = _dev(rng.uniform(size=(N, 3)).astype(np.float32), gpu)
    fb = FrameBatch(len(times), N, c["W"], c["H"], 3, gpu)
    with torch.no_grad():
        fb.render_dynamic(c["clock"], times, _dev(c["extr"], gpu), feature, position=_dev(c["position"], gpu),
                          pos_cubic_node=dy.to_segment_major(_dev(c["cubic"], gpu), I), rotation=_dev(c["rotation"], gpu),
                          rot_poly_feat=_dev(c["rot_poly"], gpu), rot_fourier_feat=_dev(c["rot_fourier"], gpu),
                          opacity=_dev(c["opacity"], gpu), scaling=_dev(c["scaling"], gpu), cubic_layout=dy.SEGMENT_MAJOR,
                          nearest=c["nearest"], extent=c["extent"])
    torch.cuda.synchronize()
    fb.check()
    rep = gr.Report(c)
    for f, t in enumerate(times):
        gr.check_chain(rep, f"batch_dyn.f{f}.", gr.chain_ref(c, dyn=(t, dy.SEGMENT_MAJOR)), _batch_buffers(fb, f))
    rep.finish()
