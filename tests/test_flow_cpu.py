"""The fifth extension header include/splat_hip_flow.h without a GPU (the mirror of tests/test_layers_cam_cpu.py): parsed on top
of the core header, exported by the built library with the parsed arity, versioned on its own, part of the build id, its
argument checks in front of any HIP call; the golden flow colours of the reference against the float64 restatement of
tests/flow_ref.py; and the Python validation of splatter_a_video_amd.flow on CPU tensors."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import flow_ref as FR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FLOW_H = os.path.join(ROOT, "include", "splat_hip_flow.h")
CSRC = os.path.join(ROOT, "splatter_a_video_amd", "csrc")
NAMES = ["splat_flow_abi_version", "splat_flow_attribute_batch", "splat_flow_attribute_batch_backward", "splat_flow_scratch_bytes",
         "splat_flow_to_image", "splat_flow_error"]
ONE = ctypes.c_void_p(16)          # never dereferenced: every call of these tests is refused on the host or launches nothing
F32 = ctypes.c_float
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "flow_wheel.npz")
CASES = ("random", "odd", "zeros", "directions", "stack", "clip", "bgr")


@pytest.fixture(scope="module")
def built_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_header_parses_on_top_of_the_core_header(built_lib):
    from splatter_a_video_amd import _abi
    L = built_lib
    h = _abi.load(FLOW_H, L.HEADER)
    assert list(h.functions) == L.FLOW_SYMBOLS == NAMES
    assert h.defines == {"SPLAT_FLOW_ABI_VERSION": 1, "SPLAT_FLOW_SCALE_PER_FRAME": 0, "SPLAT_FLOW_SCALE_WHOLE_CLIP": 1,
                         "SPLAT_FLOW_SCALE_GIVEN": 2} and L.FLOW_ABI_VERSION == 1
    assert h.structs == {}                                       # splat_camera_t is the core header's
    assert h.functions["splat_flow_abi_version"] == (ctypes.c_int, [])
    assert h.functions["splat_flow_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    fwd, bwd = h.functions["splat_flow_attribute_batch"], h.functions["splat_flow_attribute_batch_backward"]
    assert len(fwd[1]) == 17 and len(bwd[1]) == 20 and bwd[1][:15] == fwd[1][:15]
    assert fwd[1][-3:] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] and fwd[1][12:14] == [F32, F32]
    with pytest.raises(_abi.HeaderError, match="splat_flow_attribute_batch.*splat_camera_t"):
        _abi.load(FLOW_H)                                        # alone it does not parse: the camera struct is the core header's
    text = open(FLOW_H).read()
    assert '#include "splat_hip_layers_cam.h"' in text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", code)) == set(NAMES)


def test_symbol_lists_are_disjoint_and_the_earlier_headers_unchanged(built_lib):
    L = built_lib
    for other in (L.SYMBOLS, L.VIEWS_SYMBOLS, L.VIEWS_GRAD_SYMBOLS, L.CAMERA_GRAD_SYMBOLS, L.LAYERS_CAM_SYMBOLS):
        assert not set(L.FLOW_SYMBOLS) & set(other)
    assert (L.ABI_VERSION, L.VIEWS_ABI_VERSION, L.VIEWS_GRAD_ABI_VERSION, L.CAMERA_GRAD_ABI_VERSION, L.LAYERS_CAM_ABI_VERSION) \
        == (22, 1, 1, 1, 1)
    assert len(L.EXTENSIONS) == 5 and L.EXTENSIONS[-1][0] == "splat_hip_flow.h"
    assert not any("flow_attribute" in s or "flow_to_image" in s or "flow_error" in s for s in L.SYMBOLS)


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
    for name in L.FLOW_SYMBOLS:
        assert hasattr(so, name), f"{name} not exported"
        restype, argtypes = L.FLOW_HEADER.functions[name]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype
        assert _definition_arity(name) == len(argtypes), name
    assert lib.splat_flow_abi_version() == 1


def test_the_makefile_lists_the_source_and_the_header():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = next(line for line in mk.splitlines() if line.startswith("SRCS"))
    assert "flow.hip" in srcs.split()
    allsrc = next(line for line in mk.splitlines() if line.startswith("ALLSRC"))
    assert "splat_hip_flow.h" in allsrc and "$(SRCS)" in allsrc
    rule = next(line for line in mk.splitlines() if line.startswith("build/%.o:"))
    assert "splat_hip_flow.h" in rule
    assert re.search(r"^build/flow\.o: FLAGS \+= -ffp-contract=off$", mk, re.M)      # every product and sum rounded once


def test_a_library_without_the_extension_is_refused():
    code = ("import splatter_a_video_amd._lib as L\n"
            "L.FLOW_HEADER.functions['splat_flow_not_there'] = (None, [])\n"
            "try:\n    L.lib()\nexcept L.SplatError as e:\n"
            "    print('RAISED', all(s in str(e) for s in ('rebuild it', 'splat_flow_not_there', 'splat_hip_flow.h')))\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert "RAISED True" in out.stdout, out.stdout + out.stderr


def _camera(L, extr=None, intr=None, perspective=0, extr_fs=0, intr_fs=0):
    cam = L.HEADER.structs["splat_camera_t"]()
    cam.perspective, cam.extr_frame_stride, cam.intr_frame_stride = perspective, extr_fs, intr_fs
    cam.extr, cam.intr, cam.offsets = extr, intr, None
    return cam


def _ref(cam):
    return None if cam is None else ctypes.byref(cam)


def _attr(lib, cam1, cam2=None, backward=False, **k):
    a = dict(F=6, P=100, I=4, tab1=ONE, tab2=ONE, position=ONE, cubic=ONE, layout=1, W=96, H=64, zero=0, flow=ONE, g=ONE, acc=1,
             d_position=ONE, d_cubic=ONE)
    a.update(k)
    head = (a["F"], a["P"], a["I"], a["tab1"], a["tab2"], a["position"], a["cubic"], a["layout"], _ref(cam1), _ref(cam2), a["W"],
            a["H"], F32(0.01), F32(1.3), a["zero"])
    if backward:
        return lib.splat_flow_attribute_batch_backward(*head, a["g"], a["acc"], a["d_position"], a["d_cubic"], None)
    return lib.splat_flow_attribute_batch(*head, a["flow"], None)


def test_argument_validation_without_gpu(built_lib):
    L = built_lib
    lib = L.lib()
    err = lib.splat_last_error
    E_ARG = L.HEADER.defines["SPLAT_E_ARG"]
    a = 16
    ok = _camera(L, extr=a)
    for backward, who in ((False, b"splat_flow_attribute_batch:"), (True, b"splat_flow_attribute_batch_backward:")):
        call = lambda *c, **k: _attr(lib, *c, backward=backward, **k)
        assert call(None) == E_ARG == -1 and b"null camera" in err()
        assert call(_camera(L)) == E_ARG and b"null camera" in err()
        assert call(ok, _camera(L)) == E_ARG and b"null camera" in err()                      # a second camera without extr
        assert call(_camera(L, extr=a, perspective=1)) == E_ARG and b"perspective camera needs intr" in err()
        for bad in (dict(extr_fs=-16), dict(extr_fs=11), dict(extr_fs=1)):
            assert call(_camera(L, extr=a, **bad)) == E_ARG and b"camera stride" in err(), bad
        for bad in (dict(intr_fs=-4), dict(intr_fs=3)):
            assert call(_camera(L, extr=a, intr=a, perspective=1, **bad)) == E_ARG and b"camera stride" in err(), bad
        assert call(ok, _camera(L, extr=a, intr=a, perspective=1)) == E_ARG and b"both be orthographic or both pinhole" in err()
        for cam in (ok, _camera(L, extr=a, extr_fs=16), _camera(L, extr=a, intr=a, perspective=1, extr_fs=12, intr_fs=4)):
            for bad in (dict(P=-1), dict(F=-1), dict(F=65536), dict(I=0), dict(W=0), dict(H=-3)):
                assert call(cam, **bad) == E_ARG and b"sizes" in err(), bad
            assert call(cam, layout=7) == E_ARG and b"cubic_layout" in err()
            for k in ("tab1", "tab2", "position", "cubic"):
                assert call(cam, **{k: None}) == E_ARG and b"null input" in err(), k
            assert call(cam, P=0) == 0                                   # nothing to do: no HIP call
        assert who in err()
    assert _attr(lib, ok, F=0) == 0
    assert _attr(lib, ok, flow=None) == E_ARG and b"output" in err()
    assert _attr(lib, ok, flow=ctypes.c_void_p(20)) == E_ARG and b"misaligned" in err()
    assert _attr(lib, ok, backward=True, d_position=None, d_cubic=None) == 0      # nothing to add to
    assert _attr(lib, ok, backward=True, g=None) == E_ARG and b"gradient" in err()
    # colours
    def img(**k):
        a = dict(F=2, H=8, W=8, flow=ONE, clip=F32(0.0), mode=0, rad=F32(0.0), rad_out=None, out=ONE, bgr=0, scratch=ONE, nbytes=1 << 20)
        a.update(k)
        return lib.splat_flow_to_image(*[a[n] for n in ("F", "H", "W", "flow", "clip", "mode", "rad", "rad_out", "out", "bgr", "scratch",
                                                        "nbytes")], None)

    for bad in (dict(F=-1), dict(F=65536), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 16)):
        assert img(**bad) == E_ARG and b"sizes" in err(), bad
    assert img(mode=3) == E_ARG and b"scale_mode" in err()
    assert img(clip=F32(float("nan"))) == E_ARG and b"clip_flow" in err()
    for bad in (float("nan"), float("inf"), -1.0):
        assert img(mode=2, rad=F32(bad)) == E_ARG and b"rad_max_in" in err(), bad
    assert img(flow=None) == E_ARG and b"null pointer" in err()
    assert img(scratch=None) == E_ARG and b"scratch" in err()
    assert img(nbytes=4) == E_ARG and b"scratch" in err()
    assert img(F=0) == 0 and b"splat_flow_to_image:" in err()
    # error
    def e(**k):
        a = dict(F=2, H=8, W=8, pred=ONE, gt=ONE, weight=None, scale=F32(1.0), sums=ONE, grad=None, scratch=ONE, nbytes=1 << 20)
        a.update(k)
        return lib.splat_flow_error(*[a[n] for n in ("F", "H", "W", "pred", "gt", "weight", "scale", "sums", "grad", "scratch", "nbytes")],
                                    None)

    for bad in (dict(F=-1), dict(H=0), dict(W=-2)):
        assert e(**bad) == E_ARG and b"sizes" in err(), bad
    assert e(scale=F32(float("inf"))) == E_ARG and b"finite" in err()
    for k in ("pred", "gt", "sums"):
        assert e(**{k: None}) == E_ARG and b"null pointer" in err(), k
    assert e(sums=ctypes.c_void_p(20)) == E_ARG and b"misaligned" in err()
    assert e(nbytes=8) == E_ARG and b"scratch" in err()
    assert e(F=0) == 0
    assert lib.splat_flow_scratch_bytes(3, 37, 53) == 3 * 1 * 12 and lib.splat_flow_scratch_bytes(25, 480, 854) == 25 * 201 * 12
    assert lib.splat_flow_scratch_bytes(0, 8, 8) == 0


# ------------------------------------------------------------------ the wheel: golden bytes against the float64 restatement
def _maps(flow):
    """the reference's [..., H, W, 2] as [T, 2, H, W]"""
    f = flow if flow.ndim == 4 else flow[None]
    return np.ascontiguousarray(np.moveaxis(f, -1, 1))


def _case(g, name):
    flow, img = g[name + "_flow"], g[name + "_img"]
    kw = dict(scale="whole_clip" if flow.ndim == 4 else "per_frame", clip_flow=2.5 if name == "clip" else None, bgr=name == "bgr")
    return _maps(flow), (img if img.ndim == 4 else img[None]), kw


def test_wheel_table_and_margin():
    g = np.load(GOLDEN)
    assert np.array_equal(FR.WHEEL, g["wheel"]) and FR.WHEEL.shape == (55, 3)
    assert FR.STEEPEST == 64.0                                    # the 4-step green-cyan ramp
    assert 5e-4 < FR.LEVEL_MARGIN < 2e-3, FR.LEVEL_MARGIN         # about 1e-3 level: see flow_ref.py


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_against_the_reference_bytes(name):
    flow, img, kw = _case(np.load(GOLDEN), name)
    got, pre, exact, margin, _ = FR.colours(flow, **kw)
    dec = FR.decided(pre, exact, margin)
    diff = got.astype(np.int32) - img.astype(np.int32)
    print(f"{name}: {int((diff != 0).sum())} of {diff.size} bytes differ, undecided {1 - dec.mean():.3%}, exact 255: {exact.mean():.3%}")
    assert np.abs(diff).max() <= 1                                # one level at the most, on a pre-floor value next to an integer
    assert not (diff != 0)[dec].any()                             # every decided byte is the reference's
    assert 1 - dec.mean() <= 0.05
    if name == "zeros":
        assert (img == 255).all() and exact.all()


# ------------------------------------------------------------------ float64 restatements against autograd / direct sums
def test_attribute_restatement_against_torch_autograd():
    """the float64 attribute and its gradient against the same expression in float64 torch under autograd (the twin's
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
    intr = np.array([30.0, 28.0, 16.5, 12.0], np.float32)
    g = rng.normal(size=(4, N, 2))
    for k, e2, zero in ((None, None, False), (intr, None, True), (None, extr2, True), (intr, extr2, False)):
        nearest = 0.01 if k is None else 0.2
        ref = FR.attribute(clock, t1, t2, pos, cub, extr, k, e2, None, W, H, nearest, 1.3, zero, g=g)
        assert ref["cull1"].any() and not ref["cull1"].all()
        p = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
        c = torch.tensor(cub, dtype=torch.float64, requires_grad=True)
        total = 0.0
        for f in range(4):
            uvs, keeps = [], []
            for t, e in ((t1[f], extr), (t2[f], extr if e2 is None else e2)):
                seg, d, _ = clock.scalars(t)
                d = float(np.float32(d))
                cc = c.reshape(N, 4, I, 3)[:, :, seg]
                xyz = cc[:, 3] + cc[:, 2] * d + cc[:, 1] * d ** 2 + cc[:, 0] * d ** 3 + p
                et = torch.tensor(e, dtype=torch.float64)
                uv, dep = (TT.project_point_ortho(xyz, et, W, H, nearest, 1.3) if k is None
                           else TT.project_point_persp(xyz, torch.tensor(k, dtype=torch.float64), et, W, H, nearest, 1.3))
                uvs.append(uv)
                keeps.append(dep[:, 0] != 0)
            flow = uvs[1] - uvs[0]
            if zero:
                flow = flow * (keeps[0] & keeps[1])[:, None]
            np.testing.assert_allclose(flow.detach().numpy(), ref["flow"][f], rtol=1e-12, atol=1e-10)
            total = total + (flow * torch.tensor(g[f])).sum()
        total.backward()
        np.testing.assert_allclose(p.grad.numpy(), ref["d_position"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(c.grad.numpy().reshape(N, 4, I, 3), ref["d_cubic"], rtol=1e-6, atol=1e-9)


def test_error_restatement_and_zero_weight_frame():
    rng = np.random.default_rng(2)
    pred, gt = rng.normal(size=(3, 2, 5, 7)), rng.normal(size=(3, 2, 5, 7))
    w = rng.uniform(size=(3, 5, 7))
    w[1] = 0.0
    sums, grad = FR.error_sums(pred, gt, w, scale=0.5)
    p = torch.tensor(pred, requires_grad=True)
    d = p - torch.tensor(gt)
    wt = torch.tensor(w)
    l1 = (wt * d.abs().sum(1)).sum((1, 2))
    np.testing.assert_allclose(sums[:, 0], l1.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(sums[:, 1], (wt * d.norm(dim=1)).sum((1, 2)).detach().numpy(), rtol=1e-12)
    (0.5 * l1 / wt.sum((1, 2)).clamp_min(1e-30)).sum().backward()
    np.testing.assert_allclose(grad, p.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert (sums[1] == 0).all() and (grad[1] == 0).all()


# ------------------------------------------------------------------ python validation on CPU tensors
def test_python_surface_validates_before_gpu_work():
    import splatter_a_video_amd as S
    from splatter_a_video_amd import flow as FL
    from splatter_a_video_amd.dynamics import FrameClock
    from splatter_a_video_amd.losses import flow_l1
    assert S.render_flow is FL.render_flow and S.flow_to_image is FL.flow_to_image
    clock = FrameClock(12)
    pos, cub = torch.zeros(5, 3), torch.zeros(5, 4 * clock.interval_num * 3)
    with pytest.raises(ValueError, match="F >= 1 pairs"):
        FL.flow_attribute(clock, [0, 1], [1], torch.eye(4), 32, 16, position=pos, pos_cubic_node=cub)
    with pytest.raises(ValueError, match="cameras are constants"):
        FL.flow_attribute(clock, [0], [1], torch.eye(4, requires_grad=True), 32, 16, position=pos, pos_cubic_node=cub)
    with pytest.raises(ValueError, match="CUDA"):
        FL.flow_attribute(clock, [0], [1], torch.eye(4), 32, 16, position=pos, pos_cubic_node=cub)
    with pytest.raises(ValueError, match=r"\[T, 2, H, W\]"):
        FL.flow_to_image(torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError, match="CUDA"):
        FL.flow_to_image(torch.zeros(2, 2, 4, 4))
    with pytest.raises(ValueError, match="CUDA"):
        FL.flow_epe(torch.zeros(2, 2, 4, 4), torch.zeros(2, 2, 4, 4))
    with pytest.raises(ValueError, match="CUDA"):
        flow_l1(torch.zeros(2, 2, 4, 4), torch.zeros(2, 2, 4, 4))
    with pytest.raises(ValueError, match="T >= 1 pairs"):
        FL.render_flow({}, clock, [0, 1], [1], torch.eye(4), 32, 16)
