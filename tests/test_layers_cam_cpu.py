"""The fourth extension header include/splat_hip_layers_cam.h without a GPU (the mirror of tests/test_views_grad_cpu.py):
parsed on top of the core header, exported by the built library with the parsed arity, versioned on its own, disjoint from the
four lists before it, its argument checks in front of any HIP call; and the Python validation of the camera arguments of
layers / lift / views and of the forward-only frame batch on CPU tensors."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from test_layers_cpu import _model

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CAM_H = os.path.join(ROOT, "include", "splat_hip_layers_cam.h")
CSRC = os.path.join(ROOT, "splatter_a_video_amd", "csrc")
PRE = "splat_frame_preprocess_layer_batch_cam"
NAMES = ["splat_layers_cam_abi_version", PRE]
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
    h = _abi.load(CAM_H, L.HEADER)
    assert list(h.functions) == L.LAYERS_CAM_SYMBOLS == NAMES
    assert h.defines == {"SPLAT_LAYERS_CAM_ABI_VERSION": 1} and L.LAYERS_CAM_ABI_VERSION == 1
    assert h.structs == {}                                       # splat_camera_t is the core header's
    assert h.functions["splat_layers_cam_abi_version"] == (ctypes.c_int, [])
    # the argument list of the core twin with the camera struct in place of the extrinsics (both are pointers)
    core = L.HEADER.functions["splat_frame_preprocess_layer_batch"]
    assert h.functions[PRE] == core and len(core[1]) == 31
    text = open(CAM_H).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    proto = lambda src, name: re.sub(r"\s+", " ", re.search(name + r"\s*\(([^)]*)\)", src, flags=re.S)[1]).strip()
    core_code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "splat_hip.h")).read(), flags=re.S)
    assert proto(code, PRE) == proto(core_code, r"splat_frame_preprocess_layer_batch").replace("const float *extr",
                                                                                                "const splat_camera_t *cam")
    # alone it does not parse: the #include line is blanked and splat_camera_t / splat_stream_t are the core header's
    with pytest.raises(_abi.HeaderError, match=PRE + ".*splat_camera_t"):
        _abi.load(CAM_H)
    assert '#include "splat_hip_views.h"' in text
    assert set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", code)) == set(NAMES)


def test_symbol_lists_are_disjoint_and_unchanged(built_lib):
    L = built_lib
    for other in (L.SYMBOLS, L.VIEWS_SYMBOLS, L.VIEWS_GRAD_SYMBOLS, L.CAMERA_GRAD_SYMBOLS):
        assert not set(L.LAYERS_CAM_SYMBOLS) & set(other)
    assert L.VIEWS_SYMBOLS == ["splat_views_abi_version", "splat_frame_preprocess_forward_batch_cam", "splat_frames_present"]
    assert len(L.VIEWS_GRAD_SYMBOLS) == 4 and len(L.CAMERA_GRAD_SYMBOLS) == 3
    assert (L.ABI_VERSION, L.VIEWS_ABI_VERSION, L.VIEWS_GRAD_ABI_VERSION, L.CAMERA_GRAD_ABI_VERSION) == (22, 1, 1, 1)
    assert not any(s.startswith("splat_layers_cam") or s.endswith("layer_batch_cam") for s in L.SYMBOLS)


def _definition_arity(name):
    """parameters of the extern "C" definition of ``name`` in the library's sources"""
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith(".hip"):
            m = re.search(r'extern\s+"C"\s+int\s+' + name + r"\s*\(([^)]*)\)\s*\{", open(os.path.join(CSRC, fn)).read())
            if m:
                params = m[1].strip()
                return 0 if params in ("", "void") else params.count(",") + 1
    raise AssertionError(f"{name} is defined in no .hip file")


def test_symbols_exported_with_the_parsed_arity(built_lib):
    L = built_lib
    so = ctypes.CDLL(L.LIB_PATH)
    lib = L.lib()
    for name in L.LAYERS_CAM_SYMBOLS:
        assert hasattr(so, name), f"{name} not exported"
        restype, argtypes = L.LAYERS_CAM_HEADER.functions[name]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype
        assert _definition_arity(name) == len(argtypes), name
    assert lib.splat_layers_cam_abi_version() == 1


def test_the_header_is_part_of_the_build_id():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    allsrc = next(line for line in mk.splitlines() if line.startswith("ALLSRC"))
    assert "splat_hip_layers_cam.h" in allsrc and "$(SRCS)" in allsrc
    rule = next(line for line in mk.splitlines() if line.startswith("build/%.o:"))
    assert "splat_hip_layers_cam.h" in rule


def test_a_library_without_the_extension_is_refused():
    """a library that lacks an entry point of this header raises the "rebuild it" error and names the header"""
    code = ("import splatter_a_video_amd._lib as L\n"
            "L.LAYERS_CAM_HEADER.functions['splat_layers_cam_not_there'] = (None, [])\n"
            "try:\n    L.lib()\nexcept L.SplatError as e:\n"
            "    print('RAISED', all(s in str(e) for s in ('rebuild it', 'splat_layers_cam_not_there', 'splat_hip_layers_cam.h')))\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert "RAISED True" in out.stdout, out.stdout + out.stderr


def _camera(L, extr=None, intr=None, perspective=0, extr_fs=0, intr_fs=0):
    cam = L.HEADER.structs["splat_camera_t"]()
    cam.perspective, cam.extr_frame_stride, cam.intr_frame_stride = perspective, extr_fs, intr_fs
    cam.extr, cam.intr, cam.offsets = extr, intr, None
    return cam


def _pre(lib, cam, **k):
    a = dict(F=6, P=100, S=40, Q=140, q0=100, I=4, tab=ONE, src=ONE, position=ONE, cubic=ONE, layout=1, rotation=ONE, rot_poly=ONE,
             rot_fourier=ONE, opacity=ONE, scaling=ONE, W=96, H=64, centroid=None, delta=None, scale=1.0, splats=0, uv=ONE,
             depth=ONE, conic=ONE, radius=ONE, opa_t=ONE)
    a.update(k)
    return lib.splat_frame_preprocess_layer_batch_cam(
        a["F"], a["P"], a["S"], a["Q"], a["q0"], a["I"], a["tab"], a["src"], a["position"], a["cubic"], a["layout"], a["rotation"],
        a["rot_poly"], a["rot_fourier"], a["opacity"], a["scaling"], None if cam is None else ctypes.byref(cam), a["W"], a["H"],
        F32(0.01), F32(1.3), a["centroid"], a["delta"], F32(a["scale"]), a["splats"], a["uv"], a["depth"], a["conic"], a["radius"],
        a["opa_t"], None)


def test_argument_validation_without_gpu(built_lib):
    L = built_lib
    lib = L.lib()
    err = lib.splat_last_error
    E_ARG = L.HEADER.defines["SPLAT_E_ARG"]
    a = 16
    # the camera's own checks (splat_frame_preprocess_forward_batch_cam's)
    assert _pre(lib, None) == E_ARG == -1 and b"null camera" in err() and PRE.encode() + b":" in err()
    assert _pre(lib, _camera(L)) == E_ARG and b"null camera" in err()                      # cam->extr == NULL
    assert _pre(lib, _camera(L, extr=a, perspective=1)) == E_ARG and b"perspective camera needs intr" in err()
    for bad in (dict(extr_fs=-16), dict(extr_fs=11), dict(extr_fs=1)):
        assert _pre(lib, _camera(L, extr=a, **bad)) == E_ARG and b"camera stride" in err(), bad
    for bad in (dict(intr_fs=-4), dict(intr_fs=3)):
        assert _pre(lib, _camera(L, extr=a, intr=a, perspective=1, **bad)) == E_ARG and b"camera stride" in err(), bad
    # the layer entry point's checks, in front of the launch, under a per-frame and under a pinhole camera
    for cam in (_camera(L, extr=a, extr_fs=16), _camera(L, extr=a, extr_fs=12), _camera(L, extr=a, intr=a, perspective=1),
                _camera(L, extr=a, intr=a, perspective=1, extr_fs=16, intr_fs=4)):
        for bad in (dict(P=0), dict(F=-1), dict(F=65536), dict(S=-2), dict(Q=0), dict(q0=-1), dict(I=0), dict(W=0), dict(H=-3)):
            assert _pre(lib, cam, **bad) == E_ARG and b"sizes" in err(), bad
        assert _pre(lib, cam, S=101, Q=300) == E_ARG and b"at most P" in err()
        assert _pre(lib, cam, q0=101) == E_ARG and b"q0 + S" in err()
        assert _pre(lib, cam, q0=0x7fffffff, Q=0x7fffffff) == E_ARG and b"q0 + S" in err()
        assert _pre(lib, cam, layout=7) == E_ARG and b"cubic_layout" in err()
        for s in (float("nan"), float("inf")):
            assert _pre(lib, cam, scale=s, centroid=ONE) == E_ARG and b"finite" in err(), s
        assert _pre(lib, cam, scale=0.6) == E_ARG and b"centroid" in err()
        assert _pre(lib, cam, scale=0.6, delta=ONE) == E_ARG and b"centroid" in err()
        assert _pre(lib, cam, src=None) == E_ARG and b"S must be P" in err()
        for k in ("tab", "position", "cubic", "rotation", "rot_poly", "rot_fourier", "opacity", "scaling"):
            assert _pre(lib, cam, **{k: None}) == E_ARG and b"null input" in err(), k
        for k in ("uv", "depth", "conic", "radius", "opa_t"):
            assert _pre(lib, cam, **{k: None}) == E_ARG and b"null output" in err(), k
        assert PRE.encode() + b":" in err()
        # S == 0 or F == 0 is valid and launches nothing (no HIP call: this machine may have no GPU)
        assert _pre(lib, cam, S=0) == 0 and _pre(lib, cam, F=0) == 0
    # one orthographic camera is the core entry point: its own checks answer, under its own name
    for cam, k in ((_camera(L, extr=a), dict(q0=101)), (_camera(L, extr=a, extr_fs=16), dict(q0=101, F=1))):
        assert _pre(lib, cam, **k) == E_ARG and b"splat_frame_preprocess_layer_batch:" in err() and b"q0 + S" in err()
    assert _pre(lib, _camera(L, extr=a), S=0) == 0


# ------------------------------------------------------------------ python validation on CPU tensors
def test_camera_arguments_validate_before_gpu_work():
    from splatter_a_video_amd.layers import Layer, LayeredClip, add_foreground, render_part
    from splatter_a_video_amd.lift import FeatureLift, lift_features
    N, W, H = 5, 32, 16
    clock, model = _model(N)
    times, extr = [0, 1, 2], torch.eye(4)
    per = torch.eye(4)[None].repeat(3, 1, 1)
    intr = torch.tensor([20.0, 20.0, 16.0, 8.0])
    part = lambda **k: render_part(model, clock, times, k.pop("e", per), W, H, **k)
    add = lambda **k: add_foreground(model, clock, times, k.pop("e", per), W, H, (0.1, 0.0, 0.0), 0.5, **k)
    for call in (part, add):
        with pytest.raises(ValueError, match=r"per-frame extr must be \[T = 3, 4, 4\]"):
            call(e=torch.eye(4)[None].repeat(2, 1, 1))                        # a wrong T
        with pytest.raises(ValueError, match="extr"):
            call(e=torch.zeros(3, 2, 4))
        for bad in (torch.ones(3), torch.ones(2, 4), torch.ones(4, dtype=torch.float64), [1.0, 2.0, 3.0, 4.0]):
            with pytest.raises(ValueError, match="intr must be float32"):
                call(intr=bad)
            with pytest.raises(ValueError, match="intr must be float32"):
                call(e=extr, intr=bad)
        for ok in (dict(), dict(intr=intr), dict(intr=intr[None].repeat(3, 1)), dict(e=extr, intr=intr)):
            with pytest.raises(ValueError, match="CUDA"):                    # well-formed cameras still need the GPU
                call(**ok)
    # the constructors keep one camera; intr is one pinhole camera or None
    sets = [dict(feature=torch.zeros(N, 3), bg=1.0), dict(feature="depth", bg=1.0)]
    with pytest.raises(ValueError, match="extr must be one camera"):
        LayeredClip(model, clock, [Layer()], per, W, H, sets)
    for bad in (torch.ones(3, 4), torch.ones(3), torch.ones(4, dtype=torch.float64), (1.0, 2.0, 3.0, 4.0)):
        with pytest.raises(ValueError, match="intr must be None or one pinhole camera"):
            LayeredClip(model, clock, [Layer()], extr, W, H, sets, intr=bad)
        with pytest.raises(ValueError, match="intr must be None or one pinhole camera"):
            FeatureLift(model, clock, extr, W, H, 3, intr=bad)
    with pytest.raises(ValueError, match="extr must be one camera"):
        FeatureLift(model, clock, per, W, H, 3)
    with pytest.raises(ValueError, match="K > 0"):                           # contributor ids stay refused
        LayeredClip(model, clock, [Layer()], extr, W, H, sets, K=2, intr=intr)
    with pytest.raises(ValueError, match="CUDA"):
        LayeredClip(model, clock, [Layer()], extr, W, H, sets, intr=intr)
    maps = torch.zeros(3, 2, H, W)
    with pytest.raises(ValueError, match=r"per-frame extr must be \[T = 3, 4, 4\]"):
        lift_features(model, clock, times, per[:2], W, H, maps)
    with pytest.raises(ValueError, match="intr must be float32"):
        lift_features(model, clock, times, per, W, H, maps, intr=torch.ones(2, 4))
    with pytest.raises(ValueError, match="CUDA"):
        lift_features(model, clock, times, per, W, H, maps, intr=intr)


def test_views_layers_argument_validation():
    from splatter_a_video_amd.layers import Layer
    from splatter_a_video_amd.views import render_stereo, render_views
    N, W, H = 5, 32, 16
    clock, model = _model(N)
    times, per = [0, 1, 2], torch.eye(4)[None].repeat(3, 1, 1)
    wide = dict(feature=torch.zeros(N, 40), bg=0.0, detach_opacity=True)
    for bad in (dict(K=4), dict(wide=wide), dict(K=1, wide=wide)):
        with pytest.raises(ValueError, match=r"neither contributor ids \(K > 0\) nor wide= is built for layered scenes"):
            render_views(model, clock, times, per, W, H, layers=[Layer()], **bad)
    with pytest.raises(ValueError, match="layer 0: 2 times for a clip of 3 frames"):
        render_views(model, clock, times, per, W, H, layers=[Layer(times=[0, 1])])
    with pytest.raises(ValueError, match=r"per-frame extr must be \[T = 3, 4, 4\]"):
        render_views(model, clock, times, per[:2], W, H, layers=[Layer()])
    with pytest.raises(ValueError, match="CUDA"):
        render_views(model, clock, times, per, W, H, layers=[Layer()])
    with pytest.raises(ValueError, match="frames_per_batch must be an even integer"):
        render_stereo(model, clock, times, W, H, layers=[Layer()], frames_per_batch=3)
    with pytest.raises(ValueError, match="CUDA"):
        render_stereo(model, clock, times, W, H, layers=[Layer()])


def test_a_batch_without_records_refuses_a_differentiable_render():
    """the guard of FrameBatch(records=False) stands in front of everything a render does, so it answers on CPU tensors (the
    constructor needs the GPU: the object is made without it)"""
    from splatter_a_video_amd.frames import FrameBatch
    import inspect
    assert inspect.signature(FrameBatch.__init__).parameters["records"].default is True
    fb = object.__new__(FrameBatch)
    fb.records = False
    clock, model = _model(5)
    geo = {k: v for k, v in model.items() if k not in ("shs", "mask_attribute")}
    sets = [dict(feature=torch.zeros(5, 3), bg=1.0, taps=True)]
    live = dict(geo, position=geo["position"].clone().requires_grad_(True))
    with pytest.raises(ValueError, match="records=False"):
        fb.render_dynamic_sets(clock, [0], torch.eye(4), sets, **live)
    with pytest.raises(ValueError, match="records=False"):
        fb.render_dynamic_sets(clock, [0], torch.eye(4), [dict(feature=torch.zeros(5, 3, requires_grad=True), bg=1.0)], **geo)
    with pytest.raises(ValueError, match="records=False"):
        fb.render_dynamic_sets(clock, [0], torch.eye(4), sets, differentiable=True, **geo)
    with pytest.raises(ValueError, match="records=False"):
        fb.render_dynamic(clock, [0], torch.eye(4), torch.zeros(5, 3), **live)
    with pytest.raises(ValueError, match="records=False"):
        fb.render(live["position"], torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(5, 1), torch.zeros(5, 3), None, torch.eye(4))
    with pytest.raises(ValueError, match="records=False"):
        fb.render_sets(live["position"], torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(5, 1), sets, None, torch.eye(4))
    # a batch with records (the default) is not refused by the guard: the call goes on to the batch's own state
    fb.records = True
    with pytest.raises(AttributeError):
        fb.render_dynamic_sets(clock, [0], torch.eye(4), sets, differentiable=True, **geo)
