"""The camera gradients of a dynamic frame batch (include/splat_hip_camera_grad.h) without a GPU: the float64 reference of
tests/camera_grad_ref.py is finite and float32 attains its bar on every problem (pinhole: the C oracle's per-operator chain,
whose project_point / ewa_project carry the reference's dL_dintr / dL_dextr, on the oracle's dynamic evaluation; orthographic:
the twin in float32 -- the oracle has no orthographic camera gradient); the third extension header parsed, versioned,
exported and validated as tests/test_views_grad_cpu.py does it for the second; views.pose_delta."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import camera_grad_ref as cr
import gauss_backward_ref as gb
import geometry_ref as gr
import torch_twin as tw

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CAM_H = os.path.join(ROOT, "include", "splat_hip_camera_grad.h")
CSRC = os.path.join(ROOT, "splatter_a_video_amd", "csrc")
NAMES = ["splat_camera_grad_abi_version", "splat_camera_grad_partials_floats", "splat_frames_camera_backward_dynamic"]
PROBLEMS = [(m, n, k) for m, n in cr.problems() for k in cr.LAYOUTS]
IDS = [f"{m}-{n}-{k}" for m, n, k in PROBLEMS]


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("mode,name,lkey", PROBLEMS, ids=IDS)
def test_reference_is_finite_and_not_trivial(mode, name, lkey):
    P = cr.problem(mode, name, lkey)
    ref = P["ref"]
    assert torch.isfinite(ref["extr"]).all() and torch.isfinite(ref["intr"]).all()
    assert (ref["extr"].abs().amax((1, 2)) > 0).all(), "every frame's camera receives a gradient"
    if cr.MODES[mode]["ortho"]:
        assert (ref["intr"] == 0).all()
        if P["depth_channel"] < 0:
            assert (ref["extr"][:, 2] == 0).all()          # plain records: no depth gradient, the third row gets nothing
        else:
            assert (ref["extr"][:, 2].abs().amax(1) > 0).all()
    else:
        assert (ref["intr"].abs().amax(1) > 0).all()


def test_unmasked_chain_is_not_finite_for_ortho_pf():
    """a chain over ALL rows multiplies the non-finite coordinates of rows without records by a zero upstream gradient"""
    P = cr.problem("ortho_pf", "run5", "sets_wide")
    c = cr.dyn_case("ortho_pf")
    assert not np.isfinite(c["position"]).all()
    bad = cr.reference("ortho_pf", c, P["times"], P["R"], P["S"], P["depth_channel"], masked=False)
    assert not torch.isfinite(bad["extr"]).all()
    assert torch.isfinite(P["ref"]["extr"]).all()


def oracle_camera_grads(o, mode, c, times, R, S, depth_channel):
    """the float32 C oracle frame by frame: dynamic evaluation, project_point and ewa_project backward under the frame's
    camera over the rows that own records, their dL_dintr / dL_dextr added"""
    be = gr.OracleBackend(o)
    di, de = [], []
    for f, t in enumerate(times):
        intr, extr = cr.frame_camera(mode, c, f)
        idx = np.nonzero(R["cnt"][f] > 0)[0]
        up = gb.upstream(R, S, f, depth_channel)
        sc = dict(cr.subcase(c, idx), intr=intr, extr=extr)
        d = be.dyn(sc, t, tw.GAUSSIAN_MAJOR)
        p = be.project(sc, d["pos"], up["g_uv"][idx], up["g_d"][idx])
        vis = p["depth"].reshape(-1) != 0
        cov = o.compute_cov3d_forward(d["scl"], d["rot"], vis)
        e = be.ewa(sc, d["pos"], cov, p["uv"], vis, up["g_conic"][idx])
        flat = lambda a, n: np.asarray(a, np.float64).reshape(-1)[:n]
        di.append(flat(p["dintr"], 4) + flat(e["dintr"], 4))
        de.append(flat(p["dextr"], 12) + flat(e["dextr"], 12))
    return np.stack(de), np.stack(di)


@pytest.mark.parametrize("mode,name,lkey", PROBLEMS, ids=IDS)
def test_float32_attains_the_bar(oracle_mod, mode, name, lkey):
    P = cr.problem(mode, name, lkey)
    c = cr.dyn_case(mode)
    if cr.MODES[mode]["ortho"]:
        r32 = cr.reference(mode, c, P["times"], P["R"], P["S"], P["depth_channel"], dtype=torch.float32)
        extr, intr = r32["extr"].numpy(), None
    else:
        extr, intr = oracle_camera_grads(oracle_mod, mode, c, P["times"], P["R"], P["S"], P["depth_channel"])
    if cr.shared(mode):
        extr, intr = extr.sum(0), (None if intr is None else intr.sum(0))
    rep = gr.Report(P["c"])
    cr.check(rep, "f32.", extr, intr, P["ref"], cr.shared(mode))
    rep.finish()


# ------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def built_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_header_parses_on_top_of_the_core_header(built_lib):
    from splatter_a_video_amd import _abi
    L = built_lib
    h = _abi.load(CAM_H, L.HEADER)
    assert list(h.functions) == L.CAMERA_GRAD_SYMBOLS == NAMES
    assert h.defines == {"SPLAT_CAMERA_GRAD_ABI_VERSION": 1} and L.CAMERA_GRAD_ABI_VERSION == 1
    assert h.structs == {}
    i, p, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert h.functions["splat_camera_grad_abi_version"] == (i, [])
    assert h.functions["splat_camera_grad_partials_floats"] == (i64, [i, i])
    assert h.functions["splat_frames_camera_backward_dynamic"] == (
        i, [i, i, i, i, i, i64, i, i, p, p, p, p, p, i, p, p, p, p, p, p, p, p, p])
    with pytest.raises(_abi.HeaderError, match="splat_camera_t"):
        _abi.load(CAM_H)
    text = open(CAM_H).read()
    assert '#include "splat_hip_views_grad.h"' in text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", code)) == set(NAMES)


def test_older_symbol_lists_are_unchanged_and_disjoint(built_lib):
    L = built_lib
    new = set(L.CAMERA_GRAD_SYMBOLS)
    assert not new & set(L.SYMBOLS) and not new & set(L.VIEWS_SYMBOLS) and not new & set(L.VIEWS_GRAD_SYMBOLS)
    assert L.ABI_VERSION == 22 and L.VIEWS_ABI_VERSION == 1 and L.VIEWS_GRAD_ABI_VERSION == 1
    assert len(L.SYMBOLS) == 129
    assert L.VIEWS_SYMBOLS == ["splat_views_abi_version", "splat_frame_preprocess_forward_batch_cam", "splat_frames_present"]
    assert L.VIEWS_GRAD_SYMBOLS == ["splat_views_grad_abi_version", "splat_frames_gauss_backward_dynamic_cam",
                                    "splat_frames_gauss_backward_dynamic_sets_cam", "splat_frames_gauss_backward_dynamic_sources_cam"]
    assert not any("camera_grad" in s or "camera_backward" in s for s in L.SYMBOLS + L.VIEWS_SYMBOLS + L.VIEWS_GRAD_SYMBOLS)


def _definition_arity(name):
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith(".hip"):
            m = re.search(r'extern\s+"C"\s+\w+\s+' + name + r"\s*\(([^)]*)\)\s*\{", open(os.path.join(CSRC, fn)).read())
            if m:
                params = m[1].strip()
                return 0 if params in ("", "void") else params.count(",") + 1
    raise AssertionError(f"{name} is defined in no .hip file")


def test_symbols_exported_with_the_parsed_arity(built_lib):
    L = built_lib
    so = ctypes.CDLL(L.LIB_PATH)
    lib = L.lib()
    for name in L.CAMERA_GRAD_SYMBOLS:
        assert hasattr(so, name), f"{name} not exported"
        restype, argtypes = L.CAMERA_GRAD_HEADER.functions[name]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype
        assert _definition_arity(name) == len(argtypes), name
    assert lib.splat_camera_grad_abi_version() == 1
    # the caller's scratch: one row of 16 floats per workgroup of 64 Gaussians and frame, then [F,16] float64 frame sums
    assert lib.splat_camera_grad_partials_floats(1, 1) == 16 + 32
    assert lib.splat_camera_grad_partials_floats(5, 65) == 5 * 2 * 16 + 5 * 32
    assert lib.splat_camera_grad_partials_floats(0, 7) == 0 and lib.splat_camera_grad_partials_floats(3, 0) == 0


def test_the_header_is_part_of_the_build_id():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    allsrc = next(line for line in mk.splitlines() if line.startswith("ALLSRC"))
    assert "splat_hip_camera_grad.h" in allsrc and "$(SRCS)" in allsrc
    assert "cam_grad.hip" in next(line for line in mk.splitlines() if line.startswith("SRCS"))
    rule = next(line for line in mk.splitlines() if line.startswith("build/%.o:"))
    assert "splat_hip_camera_grad.h" in rule


def test_a_library_without_the_extension_is_refused():
    code = ("import splatter_a_video_amd._lib as L\n"
            "L.CAMERA_GRAD_HEADER.functions['splat_camera_grad_not_there'] = (None, [])\n"
            "try:\n    L.lib()\nexcept L.SplatError as e:\n"
            "    print('RAISED', all(s in str(e) for s in ('rebuild it', 'splat_camera_grad_not_there', 'splat_hip_camera_grad.h')))\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert "RAISED True" in out.stdout, out.stdout + out.stderr


def _camera(L, extr=None, intr=None, perspective=0, extr_fs=0, intr_fs=0):
    cam = L.HEADER.structs["splat_camera_t"]()
    cam.perspective, cam.extr_frame_stride, cam.intr_frame_stride = perspective, extr_fs, intr_fs
    cam.extr, cam.intr, cam.offsets = extr, intr, None
    return cam


def test_argument_validation_without_gpu(built_lib):
    L = built_lib
    lib = L.lib()
    E_ARG = L.HEADER.defines["SPLAT_E_ARG"]
    buf = (ctypes.c_double * 64)()                   # host memory standing in for every pointer: no check dereferences one
    a = ctypes.addressof(buf)

    def call(cam, F=2, stride=12, dcol=-1, part=a, d_extr=a, d_intr=None, layout=0):
        return lib.splat_frames_camera_backward_dynamic(F, 4, 3, 32, 32, 16, stride, dcol, a, a, a, a, a, layout, a, a, a, a, cam,
                                                        part, d_extr, d_intr, None)

    ortho, persp = _camera(L, extr=a, extr_fs=16), _camera(L, extr=a, intr=a, perspective=1, extr_fs=16, intr_fs=4)
    assert call(None) == E_ARG == -1 and b"null camera" in lib.splat_last_error()
    assert call(ctypes.byref(_camera(L))) == E_ARG and b"null camera" in lib.splat_last_error()
    assert call(ctypes.byref(_camera(L, extr=a, perspective=1))) == E_ARG and b"perspective camera needs intr" in lib.splat_last_error()
    assert call(ctypes.byref(ortho), d_intr=a) == E_ARG and b"d_intr belongs to the perspective camera" in lib.splat_last_error()
    assert call(ctypes.byref(_camera(L, extr=a, extr_fs=-16))) == E_ARG and b"negative camera stride" in lib.splat_last_error()
    assert call(ctypes.byref(_camera(L, extr=a, intr=a, perspective=1, intr_fs=-4))) == E_ARG
    assert b"negative camera stride" in lib.splat_last_error()
    for cam in (ortho, persp):
        assert call(ctypes.byref(cam), part=None) == E_ARG and b"partials" in lib.splat_last_error()
        assert call(ctypes.byref(cam), part=a + 4) == E_ARG and b"partials" in lib.splat_last_error()
        assert call(ctypes.byref(cam), dcol=12) == E_ARG and b"depth_column outside the record" in lib.splat_last_error()
        assert call(ctypes.byref(cam), dcol=40) == E_ARG
        assert call(ctypes.byref(cam), stride=10) == E_ARG and b"record_stride" in lib.splat_last_error()
        for F in (0, -3):
            assert call(ctypes.byref(cam), F=F) == E_ARG and b"bad sizes" in lib.splat_last_error()
        assert call(ctypes.byref(cam), layout=7) == E_ARG and b"unknown cubic_layout" in lib.splat_last_error()
        # both outputs NULL: nothing to do, no launch (there is no GPU here to launch on)
        assert call(ctypes.byref(cam), d_extr=None) == 0


# ------------------------------------------------------------------ views.pose_delta
def _twists(n, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([0.3 * torch.randn(n, 3, generator=g, dtype=torch.float64),
                      0.5 * torch.randn(n, 3, generator=g, dtype=torch.float64)], 1).to(dtype)


def _exp64(xi):
    wx, wy, wz, vx, vy, vz = [float(v) for v in xi]
    return torch.linalg.matrix_exp(torch.tensor([[0, -wz, wy, vx], [wz, 0, -wx, vy], [-wy, wx, 0, vz], [0, 0, 0, 0]],
                                                dtype=torch.float64))


def test_pose_delta():
    from splatter_a_video_amd import views
    extr = views.orbit_cameras(5, radius=0.3)
    same = views.pose_delta(extr, torch.zeros(5, 6))
    assert same.dtype == torch.float32 and torch.equal(same.view(torch.int32), extr.view(torch.int32))
    assert torch.equal(views.pose_delta(extr[2], torch.zeros(6)).view(torch.int32), extr[2].view(torch.int32))
    xi = _twists(5, 3, torch.float32)
    got = views.pose_delta(extr, xi)
    for f in range(5):
        want = _exp64(xi[f].double()) @ extr[f].double()
        assert (got[f].double() - want).abs().max() <= 4e-6 * want.abs().max()
        R = got[f, :3, :3].double()
        assert (R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-5       # a rigid motion stays one
        assert torch.equal(got[f, 3], extr[f, 3])
    one = views.pose_delta(extr[1], xi[1])
    assert torch.allclose(one, got[1], rtol=0, atol=1e-6)
    with pytest.raises(ValueError, match="pose_delta"):
        views.pose_delta(extr, torch.zeros(4, 6))
    with pytest.raises(ValueError, match="pose_delta"):
        views.pose_delta(extr[:, :3], torch.zeros(5, 6))


def test_pose_delta_gradcheck():
    from splatter_a_video_amd import views
    extr = views.orbit_cameras(3, radius=0.3).double().requires_grad_(True)
    xi = _twists(3, 5, torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(views.pose_delta, (extr, xi), eps=1e-6, atol=1e-6)
    assert torch.autograd.gradcheck(views.pose_delta, (extr[0].detach().requires_grad_(True), torch.zeros(6, dtype=torch.float64,
                                                                                                          requires_grad=True)),
                                    eps=1e-6, atol=1e-6)
