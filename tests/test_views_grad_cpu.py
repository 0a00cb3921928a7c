"""The second extension header include/splat_hip_views_grad.h without a GPU (the mirror of tests/test_views_cpu.py for
include/splat_hip_views.h): parsed on top of the core header, exported by the built library with the parsed arity, versioned
on its own, disjoint from the two headers before it, its argument checks in front of any HIP call."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GRAD_H = os.path.join(ROOT, "include", "splat_hip_views_grad.h")
CSRC = os.path.join(ROOT, "splatter_a_video_amd", "csrc")
NAMES = ["splat_views_grad_abi_version", "splat_frames_gauss_backward_dynamic_cam", "splat_frames_gauss_backward_dynamic_sets_cam",
         "splat_frames_gauss_backward_dynamic_sources_cam"]


@pytest.fixture(scope="module")
def built_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_header_parses_on_top_of_the_core_header(built_lib):
    from splatter_a_video_amd import _abi
    L = built_lib
    h = _abi.load(GRAD_H, L.HEADER)
    assert list(h.functions) == L.VIEWS_GRAD_SYMBOLS == NAMES
    assert h.defines == {"SPLAT_VIEWS_GRAD_ABI_VERSION": 1} and L.VIEWS_GRAD_ABI_VERSION == 1
    assert h.structs == {}                                       # splat_camera_t and splat_feature_source_t are the core's
    i, p = ctypes.c_int, ctypes.c_void_p
    i64 = ctypes.c_int64
    head = [i, i, i, i, i, i, i64]
    params = [p, p, p, p, p, p, i, p, p, p, p, p]                # records goff radius tab position cubic layout rotation .. scaling
    assert h.functions["splat_views_grad_abi_version"] == (i, [])
    assert h.functions["splat_frames_gauss_backward_dynamic_cam"] == (i, head + [i] + params + [p] + [p] * 5 + [p, p, p, p, p])
    assert h.functions["splat_frames_gauss_backward_dynamic_sets_cam"] == (
        i, head + params + [p] + [p] * 5 + [p, p, p, p, i, p, p, p, p])
    assert h.functions["splat_frames_gauss_backward_dynamic_sources_cam"] == (
        i, head + params + [p] + [p] * 5 + [i, p, i, p, p, p, p])
    # each has the argument list of its core twin with the camera struct in place of the extrinsics (both are pointers)
    for name in NAMES[1:]:
        assert h.functions[name] == L.HEADER.functions[name[:-len("_cam")]], name
    # alone it does not parse: the #include line is blanked and splat_camera_t / splat_stream_t are the core header's
    with pytest.raises(_abi.HeaderError, match="splat_frames_gauss_backward_dynamic_cam.*splat_camera_t"):
        _abi.load(GRAD_H)
    text = open(GRAD_H).read()
    assert '#include "splat_hip_views.h"' in text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", code)) == set(NAMES)


def test_symbol_lists_are_disjoint_and_unchanged(built_lib):
    L = built_lib
    assert not set(L.VIEWS_GRAD_SYMBOLS) & set(L.SYMBOLS)
    assert not set(L.VIEWS_GRAD_SYMBOLS) & set(L.VIEWS_SYMBOLS)
    assert L.VIEWS_SYMBOLS == ["splat_views_abi_version", "splat_frame_preprocess_forward_batch_cam", "splat_frames_present"]
    assert L.ABI_VERSION == 22 and L.VIEWS_ABI_VERSION == 1
    assert not any(s.startswith("splat_views_grad") or s.endswith("dynamic_cam") for s in L.SYMBOLS)


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
    for name in L.VIEWS_GRAD_SYMBOLS:
        assert hasattr(so, name), f"{name} not exported"
        restype, argtypes = L.VIEWS_GRAD_HEADER.functions[name]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype
        assert _definition_arity(name) == len(argtypes), name
    assert lib.splat_views_grad_abi_version() == 1


def test_the_header_is_part_of_the_build_id():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    allsrc = next(line for line in mk.splitlines() if line.startswith("ALLSRC"))
    assert "splat_hip_views_grad.h" in allsrc and "gauss_dyn_bwd.h" in allsrc and "$(SRCS)" in allsrc
    assert "gauss_dyn_cam.hip" in next(line for line in mk.splitlines() if line.startswith("SRCS"))


def test_a_library_without_the_extension_is_refused():
    """a library that lacks an entry point of this header raises the "rebuild it" error and names the header"""
    code = ("import splatter_a_video_amd._lib as L\n"
            "L.VIEWS_GRAD_HEADER.functions['splat_views_grad_not_there'] = (None, [])\n"
            "try:\n    L.lib()\nexcept L.SplatError as e:\n"
            "    print('RAISED', all(s in str(e) for s in ('rebuild it', 'splat_views_grad_not_there', 'splat_hip_views_grad.h')))\n")
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
    buf = (ctypes.c_float * 64)()                    # host memory standing in for every pointer: no check dereferences one
    a = ctypes.addressof(buf)
    i3 = (ctypes.c_int32 * 3)(0, 1, 2)
    p3 = (ctypes.c_void_p * 3)(a, a, a)
    table = (L.FeatureSource * L.MAX_SOURCES)()

    def plain(cam, F=2, C=3, layout=0):
        return lib.splat_frames_gauss_backward_dynamic_cam(F, 4, 3, C, 32, 32, 16, 0, a, a, a, a, a, a, layout, a, a, a, a, a, cam,
                                                           a, a, a, a, a, a, None, None, None, None)

    def sets(cam, F=2, C=4, tables=i3):
        return lib.splat_frames_gauss_backward_dynamic_sets_cam(F, 4, 3, C, 32, 32, 16, a, a, a, a, a, a, 0, a, a, a, a, a, cam,
                                                                a, a, a, a, a, tables, tables, p3, tables, -1, None, None, None, None)

    def sources(cam, F=2, C=4, nsrc=1):
        return lib.splat_frames_gauss_backward_dynamic_sources_cam(F, 4, 3, C, 32, 32, 16, a, a, a, a, a, a, 0, a, a, a, a, a, cam,
                                                                   a, a, a, a, a, nsrc, table, -1, None, None, None, None)

    for name, fn in (("dynamic_cam", plain), ("dynamic_sets_cam", sets), ("dynamic_sources_cam", sources)):
        assert fn(None) == E_ARG == -1, name
        assert b"null camera" in lib.splat_last_error()
        assert fn(ctypes.byref(_camera(L))) == E_ARG and b"null camera" in lib.splat_last_error(), name            # cam->extr == NULL
        assert fn(ctypes.byref(_camera(L, extr=a, perspective=1))) == E_ARG, name
        assert b"perspective camera needs intr" in lib.splat_last_error()
        assert fn(ctypes.byref(_camera(L, extr=a, extr_fs=-16))) == E_ARG and b"negative camera stride" in lib.splat_last_error()
        assert fn(ctypes.byref(_camera(L, extr=a, intr=a, perspective=1, intr_fs=-4))) == E_ARG
        assert b"negative camera stride" in lib.splat_last_error()
        # the checks of the core twins, in front of the launch, under a per-frame and under a pinhole camera
        for cam in (_camera(L, extr=a, extr_fs=16), _camera(L, extr=a, intr=a, perspective=1)):
            for F in (0, -3):
                assert fn(ctypes.byref(cam), F=F) == E_ARG and b"bad sizes" in lib.splat_last_error(), name
            assert fn(ctypes.byref(cam), C=33) == E_ARG and b"bad sizes" in lib.splat_last_error(), name
    per_frame = ctypes.byref(_camera(L, extr=a, extr_fs=16))
    assert plain(per_frame, layout=7) == E_ARG and b"unknown cubic_layout" in lib.splat_last_error()
    assert sets(per_frame, tables=None) == E_ARG and b"null set table" in lib.splat_last_error()
    assert sources(per_frame, nsrc=L.MAX_SOURCES + 1) == E_ARG and b"source table" in lib.splat_last_error()
    # one orthographic camera is the core entry point: its own checks answer, under its own name
    assert plain(ctypes.byref(_camera(L, extr=a)), F=0) == E_ARG
    assert b"splat_frames_gauss_backward_dynamic:" in lib.splat_last_error()
