"""The sixth extension header include/splat_hip_flow_occ.h without a GPU (the mirror of tests/test_flow_cpu.py): parsed on top of
the core header, exported by the built library with the parsed arity, versioned on its own, bound through a second tuple beside
the five frozen rows, part of the build id, its argument checks in front of any HIP call; the Python validation of
flow_occlusion / warp_by_flow / render_flow on CPU tensors; and the numpy restatements of tests/flow_occ_ref.py against an
independent statement of the sampling convention (grid_sample) and against each other."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import flow_occ_ref as OR
import flow_ref as FR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OCC_H = os.path.join(ROOT, "include", "splat_hip_flow_occ.h")
CSRC = os.path.join(ROOT, "splatter_a_video_amd", "csrc")
NAMES = ["splat_flow_occ_abi_version", "splat_flow_attribute_depth_batch", "splat_flow_attribute_depth_batch_backward",
         "splat_flow_occlusion_scratch_bytes", "splat_flow_occlusion"]
DEFINES = {"SPLAT_FLOW_OCC_ABI_VERSION": 1, "SPLAT_FLOW_OCC_OUTSIDE": 1, "SPLAT_FLOW_OCC_UNCOVERED": 2, "SPLAT_FLOW_OCC_IN_FRONT": 4,
           "SPLAT_FLOW_OCC_INCONSISTENT": 8}
ONE = ctypes.c_void_p(16)          # never dereferenced: every call of these tests is refused on the host or launches nothing
F32 = ctypes.c_float


@pytest.fixture(scope="module")
def built_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_header_parses_on_top_of_the_core_header(built_lib):
    from splatter_a_video_amd import _abi
    L = built_lib
    h = _abi.load(OCC_H, L.HEADER)
    assert list(h.functions) == L.FLOW_OCC_SYMBOLS == NAMES
    assert h.defines == DEFINES and L.FLOW_OCC_ABI_VERSION == 1
    assert h.structs == {}
    assert h.functions["splat_flow_occ_abi_version"] == (ctypes.c_int, [])
    assert h.functions["splat_flow_occlusion_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    # the attribute with the depth takes the two-channel entry points' arguments, the stream last
    for new, old in (("splat_flow_attribute_depth_batch", "splat_flow_attribute_batch"),
                     ("splat_flow_attribute_depth_batch_backward", "splat_flow_attribute_batch_backward")):
        assert h.functions[new] == L.FLOW_HEADER.functions[old]
    occ = h.functions["splat_flow_occlusion"]
    assert occ[0] is ctypes.c_int and len(occ[1]) == 23 and occ[1][:4] == [ctypes.c_int] * 4 and occ[1][10:15] == [F32] * 5
    assert occ[1][-2:] == [ctypes.c_size_t, ctypes.c_void_p]
    with pytest.raises(_abi.HeaderError, match="splat_camera_t"):
        _abi.load(OCC_H)                                          # alone it does not parse: the camera struct is the core header's
    text = open(OCC_H).read()
    assert '#include "splat_hip_flow.h"' in text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", code)) == set(NAMES)
    from splatter_a_video_amd import flow as FL
    assert (FL.OUTSIDE, FL.UNCOVERED, FL.IN_FRONT, FL.INCONSISTENT) == (1, 2, 4, 8) == (OR.OUTSIDE, OR.UNCOVERED, OR.IN_FRONT,
                                                                                      OR.INCONSISTENT)


def test_bound_beside_the_five_frozen_rows(built_lib):
    L = built_lib
    assert len(L.EXTENSIONS) == 5 and L.EXTENSIONS[-1][0] == "splat_hip_flow.h"
    assert L.LATER_EXTENSIONS == (("splat_hip_flow_occ.h", "SPLAT_FLOW_OCC_ABI_VERSION", "splat_flow_occ_abi_version"),)
    assert (L.ABI_VERSION, L.VIEWS_ABI_VERSION, L.VIEWS_GRAD_ABI_VERSION, L.CAMERA_GRAD_ABI_VERSION, L.LAYERS_CAM_ABI_VERSION,
            L.FLOW_ABI_VERSION) == (22, 1, 1, 1, 1, 1)
    for other in (L.SYMBOLS, L.VIEWS_SYMBOLS, L.VIEWS_GRAD_SYMBOLS, L.CAMERA_GRAD_SYMBOLS, L.LAYERS_CAM_SYMBOLS, L.FLOW_SYMBOLS):
        assert not set(L.FLOW_OCC_SYMBOLS) & set(other)


def _definition_arity(name):
    text = open(os.path.join(CSRC, "flow.hip")).read()
    m = re.search(r'extern\s+"C"\s+\w+\s+' + name + r"\s*\(([^)]*)\)\s*\{", text)
    assert m, f"{name} is not defined in flow.hip"
    params = m[1].strip()
    return 0 if params in ("", "void") else params.count(",") + 1


def test_symbols_exported_with_the_parsed_arity(built_lib):
    L = built_lib
    so = ctypes.CDLL(L.LIB_PATH)
    lib = L.lib()
    for name in NAMES:
        assert hasattr(so, name), f"{name} not exported"
        restype, argtypes = L.FLOW_OCC_HEADER.functions[name]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype
        assert _definition_arity(name) == len(argtypes), name
    assert lib.splat_flow_occ_abi_version() == 1


def test_the_makefile_lists_the_header():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    allsrc = next(line for line in mk.splitlines() if line.startswith("ALLSRC"))
    assert "splat_hip_flow_occ.h" in allsrc                       # part of the build id
    rule = next(line for line in mk.splitlines() if line.startswith("build/%.o:"))
    assert "splat_hip_flow_occ.h" in rule
    assert re.search(r"^build/flow\.o: FLAGS \+= -ffp-contract=off$", mk, re.M)      # the new kernels live in flow.hip


def test_a_library_without_the_extension_is_refused():
    code = ("import splatter_a_video_amd._lib as L\n"
            "L.FLOW_OCC_HEADER.functions['splat_flow_occ_not_there'] = (None, [])\n"
            "try:\n    L.lib()\nexcept L.SplatError as e:\n"
            "    print('RAISED', all(s in str(e) for s in ('rebuild it', 'splat_flow_occ_not_there', 'splat_hip_flow_occ.h')))\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert "RAISED True" in out.stdout, out.stdout + out.stderr


def _camera(L, extr=None, intr=None, perspective=0):
    cam = L.HEADER.structs["splat_camera_t"]()
    cam.perspective, cam.extr_frame_stride, cam.intr_frame_stride = perspective, 0, 0
    cam.extr, cam.intr, cam.offsets = extr, intr, None
    return cam


def _attr(lib, cam1, backward=False, **k):
    a = dict(F=6, P=100, I=4, tab1=ONE, tab2=ONE, position=ONE, cubic=ONE, layout=1, W=96, H=64, zero=0, out=ONE, g=ONE, acc=1,
             d_position=ONE, d_cubic=ONE)
    a.update(k)
    head = (a["F"], a["P"], a["I"], a["tab1"], a["tab2"], a["position"], a["cubic"], a["layout"],
            None if cam1 is None else ctypes.byref(cam1), None, a["W"], a["H"], F32(0.01), F32(1.3), a["zero"])
    if backward:
        return lib.splat_flow_attribute_depth_batch_backward(*head, a["g"], a["acc"], a["d_position"], a["d_cubic"], None)
    return lib.splat_flow_attribute_depth_batch(*head, a["out"], None)


def _occ(lib, **k):
    a = dict(F=2, H=8, W=8, C=0, flow=ONE, track_depth=None, surface=None, coverage=None, flow_back=None, src=None, bg=F32(1.0),
             margin=F32(0.05), min_cov=F32(0.5), alpha=F32(0.01), beta=F32(0.5), mask=ONE, depth_gap=None, fb_sq=None, warped=None,
             counts=None, scratch=None, nbytes=0)
    a.update(k)
    return lib.splat_flow_occlusion(*[a[n] for n in ("F", "H", "W", "C", "flow", "track_depth", "surface", "coverage", "flow_back",
                                                     "src", "bg", "margin", "min_cov", "alpha", "beta", "mask", "depth_gap", "fb_sq",
                                                     "warped", "counts", "scratch", "nbytes")], None)


def test_argument_validation_without_gpu(built_lib):
    L = built_lib
    lib = L.lib()
    err = lib.splat_last_error
    E_ARG = L.HEADER.defines["SPLAT_E_ARG"]
    ok = _camera(L, extr=16)
    for backward, who in ((False, b"splat_flow_attribute_depth_batch:"), (True, b"splat_flow_attribute_depth_batch_backward:")):
        call = lambda *c, **k: _attr(lib, *c, backward=backward, **k)
        assert call(None) == E_ARG == -1 and b"null camera" in err() and who in err()
        assert call(_camera(L, extr=16, perspective=1)) == E_ARG and b"perspective camera needs intr" in err()
        for bad in (dict(P=-1), dict(F=-1), dict(F=65536), dict(I=0), dict(W=0), dict(H=-3)):
            assert call(ok, **bad) == E_ARG and b"sizes" in err() and who in err(), bad
        assert call(ok, layout=7) == E_ARG and b"cubic_layout" in err()
        for k in ("tab1", "tab2", "position", "cubic"):
            assert call(ok, **{k: None}) == E_ARG and b"null input" in err(), k
        assert call(ok, P=0) == 0                                        # nothing to do: no HIP call
    assert _attr(lib, ok, F=0) == 0
    assert _attr(lib, ok, out=None) == E_ARG and b"output" in err()
    assert _attr(lib, ok, out=ctypes.c_void_p(24)) == E_ARG and b"16-byte" in err()          # 8-byte aligned is not enough
    assert _attr(lib, ok, backward=True, d_position=None, d_cubic=None) == 0                 # nothing to add to
    assert _attr(lib, ok, backward=True, g=None) == E_ARG and b"gradient" in err()
    assert _attr(lib, ok, backward=True, g=ctypes.c_void_p(24)) == E_ARG and b"16-byte" in err()
    # the fused kernel: every refusal on the host
    who = b"splat_flow_occlusion:"
    for bad in (dict(F=-1), dict(F=65536), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 16)):
        assert _occ(lib, **bad) == E_ARG and b"sizes" in err() and who in err(), bad
    assert _occ(lib, track_depth=ONE) == E_ARG and b"both or neither" in err()               # the pair given half
    assert _occ(lib, surface=ONE) == E_ARG and b"both or neither" in err()
    for C in (0, 9, -1):
        assert _occ(lib, src=ONE, warped=ONE, C=C) == E_ARG and b"1 <= C <= 8" in err(), C
    assert _occ(lib, C=3) == E_ARG and b"C == 0 without src" in err()
    assert _occ(lib, depth_gap=ONE) == E_ARG and b"depth_gap needs" in err()
    assert _occ(lib, fb_sq=ONE) == E_ARG and b"fb_sq needs" in err()
    assert _occ(lib, src=ONE, C=3) == E_ARG and b"warped and src" in err()
    assert _occ(lib, margin=F32(float("nan"))) == E_ARG and b"NaN" in err()
    assert _occ(lib, flow=None) == E_ARG and b"null pointer" in err()
    assert _occ(lib, mask=None) == E_ARG and b"null pointer" in err()
    assert _occ(lib, flow=ctypes.c_void_p(18)) == E_ARG and b"misaligned" in err()
    assert _occ(lib, counts=ONE) == E_ARG and b"scratch" in err()
    assert _occ(lib, counts=ONE, scratch=ONE, nbytes=8) == E_ARG and b"scratch" in err() and who in err()
    assert _occ(lib, F=0) == 0 and _occ(lib, F=0, track_depth=ONE) == E_ARG                  # the pairing rule holds for F = 0 too
    assert lib.splat_flow_occlusion_scratch_bytes(3, 45, 53) == 3 * 2 * 16
    assert lib.splat_flow_occlusion_scratch_bytes(25, 480, 854) == 25 * 201 * 16
    assert lib.splat_flow_occlusion_scratch_bytes(0, 8, 8) == 0 == lib.splat_flow_occlusion_scratch_bytes(2, 0, 8)


# ------------------------------------------------------------------ python validation on CPU tensors
def test_python_surface_validates_before_gpu_work():
    import splatter_a_video_amd as S
    from splatter_a_video_amd import flow as FL
    from splatter_a_video_amd.dynamics import FrameClock
    assert S.flow_occlusion is FL.flow_occlusion and S.warp_by_flow is FL.warp_by_flow
    assert FL.FlowOcclusion._fields == ("mask", "depth_gap", "fb_sq", "warped", "counts")
    flow, plane = torch.zeros(2, 2, 4, 5), torch.zeros(2, 4, 5)
    with pytest.raises(ValueError, match=r"\[T, 2, H, W\]"):
        FL.flow_occlusion(torch.zeros(2, 3, 4, 5))
    with pytest.raises(ValueError, match="both or neither"):
        FL.flow_occlusion(flow, track_depth=plane)
    with pytest.raises(ValueError, match="both or neither"):
        FL.flow_occlusion(flow, surface_depth=plane)
    with pytest.raises(ValueError, match="flow_back must have the flow's shape"):
        FL.flow_occlusion(flow, flow_back=torch.zeros(2, 2, 4, 4))
    for C in (0, 9):
        with pytest.raises(ValueError, match="1 <= C <= 8"):
            FL.flow_occlusion(flow, src=torch.zeros(2, C, 4, 5))
    with pytest.raises(ValueError, match="1 <= C <= 8"):
        FL.warp_by_flow(torch.zeros(2, 9, 4, 5), flow)
    with pytest.raises(ValueError, match=r"coverage must be \[T, H, W\]"):
        FL.flow_occlusion(flow, coverage=torch.zeros(2, 5, 4))
    with pytest.raises(ValueError, match="CUDA"):
        FL.flow_occlusion(flow, track_depth=plane, surface_depth=plane, coverage=plane)
    with pytest.raises(ValueError, match="CUDA"):
        FL.warp_by_flow(torch.zeros(2, 3, 4, 5), flow)
    clock = FrameClock(12)
    with pytest.raises(ValueError, match="cycle=True needs occlusion=True"):
        FL.render_flow({}, clock, [0], [1], torch.eye(4), 32, 16, cycle=True)
    with pytest.raises(ValueError, match="not differentiable"):
        FL.render_flow({}, clock, [0], [1], torch.eye(4), 32, 16, occlusion=True, differentiable=True)
    pos, cub = torch.zeros(5, 3), torch.zeros(5, 4 * clock.interval_num * 3)
    with pytest.raises(ValueError, match="CUDA"):
        FL.flow_attribute(clock, [0], [1], torch.eye(4), 32, 16, position=pos, pos_cubic_node=cub, depth=True)


# ------------------------------------------------------------------ the restatements: convention and precision
HS, WS = 45, 53


def _random_lookup(seed, n=4000):
    rng = np.random.default_rng(seed)
    plane = rng.normal(0, 2.0, size=(HS, WS)).astype(np.float32)
    qx = rng.uniform(0, WS - 1, n).astype(np.float32)
    qy = rng.uniform(0, HS - 1, n).astype(np.float32)
    qx[:8], qy[:8] = [0, WS - 1, WS - 1, 0, 7, WS - 1, 3.5, WS - 2], [0, HS - 1, 0, HS - 1, HS - 1, 11.25, HS - 1, HS - 2]      # corners, edges
    return plane, qx, qy


def test_sampling_convention_is_grid_sample_align_corners():
    """q is a pixel INDEX (pixel i's centre is index i): the float64 twin's B(plane, q) is torch's grid_sample with
    align_corners=True on q normalised by (W - 1) and (H - 1) -- an independent statement of the convention"""
    plane, qx, qy = _random_lookup(0)
    got, _ = OR.bilinear(plane, qx, qy, np.float64)
    gx = 2.0 * torch.tensor(qx, dtype=torch.float64) / (WS - 1) - 1.0
    gy = 2.0 * torch.tensor(qy, dtype=torch.float64) / (HS - 1) - 1.0
    want = torch.nn.functional.grid_sample(torch.tensor(plane, dtype=torch.float64)[None, None], torch.stack([gx, gy], -1)[None, None],
                                           mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, 0].numpy()
    err = np.abs(got - want)
    print(f"B against grid_sample: max err {err.max():.3e}")
    assert err.max() <= 1e-12
    # and the rescaled convention of tracking.sample_coords is another one: it does not pass this pin
    other = torch.nn.functional.grid_sample(torch.tensor(plane, dtype=torch.float64)[None, None],
                                            torch.stack([gx * (WS - 1) / WS, gy * (HS - 1) / HS], -1)[None, None], mode="bilinear",
                                            padding_mode="zeros", align_corners=True)[0, 0, 0].numpy()
    assert np.abs(got - other).max() > 1e-2


def test_float32_restatement_stays_next_to_the_float64_twin():
    """on the same float32 q: fx = qx - floor(qx) is exact, 1 - fx, the four products and three sums round once each (two
    nested levels of three roundings on top of 1 - f): within 8 EPS (|v00| + |v01| + |v10| + |v11|)"""
    plane, qx, qy = _random_lookup(1)
    b32, mag = OR.bilinear(plane, qx, qy, np.float32)
    b64, _ = OR.bilinear(plane, qx, qy, np.float64)
    assert b32.dtype == np.float32
    ratio = np.abs(b32.astype(np.float64) - b64) / (8 * OR.EPS * mag.astype(np.float64))
    print(f"float32 B against float64: max err / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    # an integer q returns the sample itself, in both
    xi, yi = np.arange(WS, dtype=np.float32), np.full(WS, 7, np.float32)
    assert np.array_equal(OR.bilinear(plane, xi, yi, np.float32)[0], plane[7])


def test_restated_kernel_decisions_on_planted_pixels():
    """the float32 restatement on a small hand-made case: every bit where it is planted, nothing sampled outside"""
    H, W = 4, 6
    flow = np.zeros((1, 2, H, W), np.float32)
    flow[0, 0, 0, 0] = -0.5                     # leaves on the left
    flow[0, 1, 3, 2] = 0.25                     # leaves at the bottom
    flow[0, 0, 1, 1] = np.nan
    flow[0, 1, 2, 2] = np.inf
    flow[0, 0, 0, 3] = 2.0                      # (3, 0) -> (5, 0): exactly on W - 1, inside
    cov = np.ones((1, H, W), np.float32)
    cov[0, 1, 4], cov[0, 1, 5] = 0.25, 0.5      # below and exactly at min_coverage
    surface = np.full((1, H, W), 3.0, np.float32)
    surface[0, 2, 4] = 2.0                      # something nearer at (4, 2)
    track = np.full((1, H, W), 3.0, np.float32)
    back = np.zeros_like(flow)
    back[0, 0, 0, 5] = -2.0                     # the way back from (5, 0) returns to (3, 0)
    back[0, 0, 2, 0] = 3.0                      # the way back from (0, 2) does not return
    src = np.arange(H * W, dtype=np.float32).reshape(1, 1, H, W)
    r = OR.occlusion(flow, track, surface, cov, back, src, bg_depth=1.0, depth_margin=0.5, min_coverage=0.5, fb_alpha=0.01, fb_beta=0.5)
    want = np.zeros((H, W), np.uint8)
    want[0, 0] = want[3, 2] = want[1, 1] = want[2, 2] = OR.OUTSIDE
    want[1, 4] = OR.UNCOVERED
    want[2, 4] = OR.IN_FRONT
    want[2, 0] = want[0, 5] = OR.INCONSISTENT     # (5, 0) itself stays, and its way back leaves
    assert np.array_equal(r["mask"][0], want), r["mask"][0]
    assert r["counts"].tolist() == [[4, 1, 1, 2]]
    out = want == OR.OUTSIDE
    assert not r["depth_gap"][0][out].any() and not r["fb_sq"][0][out].any() and not r["warped"][0, 0][out].any()
    assert r["depth_gap"][0, 2, 4] == 1.0 and r["depth_gap"][0, 1, 4] == 0.75 and r["fb_sq"][0, 2, 0] == 9.0
    assert r["warped"][0, 0, 0, 3] == src[0, 0, 0, 5] and np.array_equal(r["warped"][0, 0][~out & (flow[0, 0] == 0)],
                                                                         src[0, 0][~out & (flow[0, 0] == 0)])
    twin = OR.occlusion(flow, track, surface, cov, back, src, bg_depth=1.0, depth_margin=0.5, min_coverage=0.5, dt=np.float64)
    assert np.array_equal(twin["mask"], r["mask"])


def test_attribute_restatement_against_torch_autograd():
    """the float64 depth channels and their gradient against the same expression in float64 torch under autograd (the twin's
    projection rules), orthographic and pinhole, a second camera, both zero_culled settings"""
    import torch_twin as TT
    from splatter_a_video_amd.dynamics import FrameClock
    rng = np.random.default_rng(5)
    N, W, H = 40, 32, 24
    clock = FrameClock(12)
    I = clock.interval_num
    pos = np.concatenate([rng.uniform(-1.6, 1.6, (N, 2)), rng.uniform(1.0, 3.0, (N, 1))], 1).astype(np.float32)
    cub = rng.normal(0, 0.05, (N, 4 * I * 3)).astype(np.float32)
    t1, t2 = [0, 3.5, 7, 11], [2, 9.25, 7, 4]
    extr = np.eye(4, dtype=np.float32)
    extr[:3, 3] = (0.05, -0.02, 0.1)
    extr2 = extr.copy()
    extr2[0, 3] += 0.2
    extr2[2, :3] = (0.1, 0.0, 0.995)
    intr = np.array([30.0, 28.0, 16.5, 12.0], np.float32)
    g = rng.normal(size=(4, N, 4))
    for k, e2, zero in ((None, None, False), (intr, None, True), (None, extr2, True), (intr, extr2, False)):
        nearest = 0.01 if k is None else 0.2
        ref = OR.attribute4(clock, t1, t2, pos, cub, extr, k, e2, None, W, H, nearest, 1.3, zero, g=g)
        two = FR.attribute(clock, t1, t2, pos, cub, extr, k, e2, None, W, H, nearest, 1.3, zero)
        assert np.array_equal(ref["attr"][..., :2], two["flow"]) and ref["cull1"].any() and not ref["cull1"].all()
        p = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
        c = torch.tensor(cub, dtype=torch.float64, requires_grad=True)
        total = 0.0
        for f in range(4):
            rows, keeps = [], []
            for t, e in ((t1[f], extr), (t2[f], extr if e2 is None else e2)):
                seg, d, _ = clock.scalars(t)
                d = float(np.float32(d))
                cc = c.reshape(N, 4, I, 3)[:, :, seg]
                xyz = cc[:, 3] + cc[:, 2] * d + cc[:, 1] * d ** 2 + cc[:, 0] * d ** 3 + p
                et = torch.tensor(e, dtype=torch.float64)
                uv, dep = (TT.project_point_ortho(xyz, et, W, H, nearest, 1.3) if k is None
                           else TT.project_point_persp(xyz, torch.tensor(k, dtype=torch.float64), et, W, H, nearest, 1.3))
                rows.append(torch.cat([uv, dep[:, :1]], 1))                # the twin zeroes uv and depth of a culled point
                keeps.append(dep[:, 0] != 0)
            attr = torch.cat([rows[1] - rows[0], rows[1][:, 2:3]], 1)
            if zero:
                attr = attr * (keeps[0] & keeps[1])[:, None]
            np.testing.assert_allclose(attr.detach().numpy(), ref["attr"][f], rtol=1e-12, atol=1e-10)
            total = total + (attr * torch.tensor(g[f])).sum()
        total.backward()
        np.testing.assert_allclose(p.grad.numpy(), ref["d_position"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(c.grad.numpy().reshape(N, 4, I, 3), ref["d_cubic"], rtol=1e-6, atol=1e-9)
        assert (ref["bound"][..., 2:] >= 0).all() and ref["bound"][..., 3].max() < 1e-4       # N_ROUND_Z EPS A_z with |z| of a few units

