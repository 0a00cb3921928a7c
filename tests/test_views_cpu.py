"""Novel views and stereo without a GPU: the extension header include/splat_hip_views.h (parsed on top of the core header,
exported by the built library, versioned on its own, its argument checks in front of any HIP call), the cameras of
splatter_a_video_amd.views against a numpy restatement with the look-at of shims/pytorch3d, and the float32 restatement of
the anaglyph mix (tests/views_ref.py) against the reference's float64 formula."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import views_ref as VR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
VIEWS_H = os.path.join(ROOT, "include", "splat_hip_views.h")
CSRC = os.path.join(ROOT, "splatter_a_video_amd", "csrc")


@pytest.fixture(scope="module")
def built_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "-j8"])
    import splatter_a_video_amd._lib as L
    return L


# ------------------------------------------------------------------ the extension header
def test_extension_header_parses_on_top_of_the_core_header(built_lib):
    from splatter_a_video_amd import _abi
    L = built_lib
    h = _abi.load(VIEWS_H, L.HEADER)
    assert list(h.functions) == L.VIEWS_SYMBOLS == ["splat_views_abi_version", "splat_frame_preprocess_forward_batch_cam",
                                                     "splat_frames_present"]
    assert h.defines == {"SPLAT_VIEWS_ABI_VERSION": 1} and L.VIEWS_ABI_VERSION == 1
    assert h.structs == {}                                       # it brings no struct of its own: splat_camera_t is the core's
    i, f, p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    assert h.functions["splat_views_abi_version"] == (i, [])
    assert h.functions["splat_frame_preprocess_forward_batch_cam"] == (
        i, [i, i, i, p, p, p, i, p, p, p, p, p, p, i, i, f, f, p, p, p, p, p, p])
    assert h.functions["splat_frames_present"] == (i, [i, i, i, p, p, p, p, p])
    # alone it does not parse: the #include line is blanked and splat_camera_t / splat_stream_t are the core header's
    with pytest.raises(_abi.HeaderError, match="splat_frame_preprocess_forward_batch_cam.*splat_camera_t"):
        _abi.load(VIEWS_H)
    # the raw text, comments included, names exactly these functions (the rule the core header is held to)
    declared = set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", open(VIEWS_H).read()))
    assert declared == set(L.VIEWS_SYMBOLS)


def test_core_binding_is_what_the_core_header_gives(built_lib):
    from splatter_a_video_amd import _abi
    L = built_lib
    core = _abi.load(os.path.join(ROOT, "include", "splat_hip.h"))
    assert L.SYMBOLS == list(core.functions) and L.HEADER.functions == core.functions
    assert L.ABI_VERSION == core.defines["SPLAT_ABI_VERSION"]
    assert not set(L.SYMBOLS) & set(L.VIEWS_SYMBOLS)
    assert "splat_stream_t" in core.handles
    assert set(core.structs) == set(L.HEADER.structs)


def _definition_arity(name):
    """parameters of the extern "C" definition of ``name`` in the library's sources"""
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith(".hip"):
            m = re.search(r'extern\s+"C"\s+int\s+' + name + r"\s*\(([^)]*)\)\s*\{", open(os.path.join(CSRC, fn)).read())
            if m:
                params = m[1].strip()
                return 0 if params in ("", "void") else params.count(",") + 1
    raise AssertionError(f"{name} is defined in no .hip file")


def test_views_symbols_exported_with_the_parsed_arity(built_lib):
    L = built_lib
    so = ctypes.CDLL(L.LIB_PATH)
    lib = L.lib()
    for name in L.VIEWS_SYMBOLS:
        assert hasattr(so, name), f"{name} not exported"
        restype, argtypes = L.VIEWS_HEADER.functions[name]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype
        assert _definition_arity(name) == len(argtypes), name
    assert lib.splat_views_abi_version() == 1


def test_a_library_without_the_extension_is_refused(tmp_path):
    """a library that lacks the extension's entry points raises the "rebuild it" error instead of binding half an ABI"""
    import sys
    code = ("import splatter_a_video_amd._lib as L\n"
            "L.VIEWS_HEADER.functions['splat_views_not_there'] = (None, [])\n"
            "try:\n    L.lib()\nexcept L.SplatError as e:\n    print('RAISED', 'rebuild it' in str(e) and 'splat_views_not_there' in str(e))\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert "RAISED True" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ argument checks in front of any HIP call
def _camera(L, extr=None, intr=None, perspective=0, extr_fs=0):
    cam = L.HEADER.structs["splat_camera_t"]()
    cam.perspective, cam.extr_frame_stride, cam.intr_frame_stride = perspective, extr_fs, 0
    cam.extr, cam.intr, cam.offsets = extr, intr, None
    return cam


def test_argument_validation_without_gpu(built_lib):
    L = built_lib
    lib = L.lib()
    buf = (ctypes.c_float * 64)()                    # host memory standing in for every pointer: no check dereferences one
    a = ctypes.addressof(buf)
    pre = lambda F, cam: lib.splat_frame_preprocess_forward_batch_cam(F, 4, 3, a, a, a, 0, a, a, a, a, a, cam, 32, 32, 0.01, 1.3,
                                                                      a, a, a, a, a, None)
    assert pre(2, None) == L.HEADER.defines["SPLAT_E_ARG"] == -1
    assert b"splat_frame_preprocess_forward_batch_cam" in lib.splat_last_error() and b"null camera" in lib.splat_last_error()
    assert pre(2, ctypes.byref(_camera(L))) == -1 and b"null camera" in lib.splat_last_error()            # cam->extr == NULL
    assert pre(2, ctypes.byref(_camera(L, extr=a, perspective=1))) == -1
    assert b"perspective camera needs intr" in lib.splat_last_error()
    for F in (0, -3):
        assert pre(F, ctypes.byref(_camera(L, extr=a))) == -1 and b"bad sizes" in lib.splat_last_error()
    assert pre(2, ctypes.byref(_camera(L, extr=a, extr_fs=-16))) == -1 and b"negative camera stride" in lib.splat_last_error()
    present = lambda F, H, W, b=None, mix=None: lib.splat_frames_present(F, H, W, a, b, mix, a, None)
    for F, H, W in ((1, 0, 8), (1, 8, 0), (1, -2, 8), (0, 8, 8)):
        assert present(F, H, W) == -1
        assert b"splat_frames_present" in lib.splat_last_error() and b"bad sizes" in lib.splat_last_error()
    assert present(1, 46341, 46341) == -1 and b"bad sizes" in lib.splat_last_error()                      # H * W past 2^31
    assert present(1, 8, 8, b=a) == -1 and b"mix matrix" in lib.splat_last_error()
    assert lib.splat_frames_present(1, 8, 8, None, None, None, a, None) == -1 and b"null pointer" in lib.splat_last_error()


def test_views_refuse_cpu_tensors(built_lib):
    from splatter_a_video_amd import views as V
    with pytest.raises(ValueError, match="CUDA"):
        V.to_uint8(torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError, match="3 x 6"):
        V.anaglyph(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), mode=torch.zeros(2, 9))
    with pytest.raises(ValueError, match="unknown anaglyph mode"):
        V.anaglyph(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), mode="cyan")


# ------------------------------------------------------------------ cameras
def _shim_look_at():
    spec = importlib.util.spec_from_file_location("_shim_pytorch3d_renderer", os.path.join(ROOT, "shims", "pytorch3d", "renderer", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.look_at_rotation


def _extr_ref(pos, at):
    """inv([look_at_rotation(pos, at) | pos]) as the reference builds it: the float32 rotation into a float64 c2w, numpy's inverse"""
    R = _shim_look_at()(torch.tensor([pos], dtype=torch.float32), at=(at,))[0].numpy()
    c2w = np.concatenate([np.concatenate([R, np.array(pos, np.float32)[:, None]], axis=1).astype(np.float64),
                          np.array([[0, 0, 0, 1.0]])], axis=0)
    return np.linalg.inv(c2w)


@pytest.mark.parametrize("n,radius,z_center,turns", [(30, 0.05, 1.0, 2.0), (7, 0.3, 2.5, 0.5), (1, 0.05, 1.0, 2.0)])
def test_orbit_cameras(n, radius, z_center, turns):
    from splatter_a_video_amd.views import orbit_cameras
    extr = orbit_cameras(n, radius, z_center, turns)
    assert extr.shape == (n, 4, 4) and extr.dtype == torch.float32
    phi = torch.linspace(0, 2 * np.pi * turns, n)
    for i in range(n):
        pos = [float(radius * torch.cos(phi[i])), float(radius * torch.sin(phi[i])), 0.0]
        np.testing.assert_allclose(extr[i].numpy(), _extr_ref(pos, (0, 0, z_center)), rtol=0, atol=1e-6)
    # world to camera: the camera's own position maps to the origin, the target onto the +z axis
    e = extr.double()
    pos = torch.stack((radius * torch.cos(phi), radius * torch.sin(phi), torch.zeros(n)), 1).double()
    assert float((torch.einsum("nij,nj->ni", e[:, :3, :3], pos) + e[:, :3, 3]).abs().max()) < 1e-6
    tgt = e[:, :3, :3] @ torch.tensor([0, 0, z_center], dtype=torch.float64) + e[:, :3, 3]
    assert float(tgt[:, :2].abs().max()) < 1e-6 and bool((tgt[:, 2] > 0).all())
    if n == 30:
        assert not torch.equal(extr[1], extr[2])


def test_stereo_cameras():
    from splatter_a_video_amd.views import stereo_cameras
    extr = stereo_cameras()
    assert extr.shape == (2, 4, 4)
    for i, phi in enumerate((0.0, np.pi)):
        pos = [0.05 * np.cos(phi), 0.05 * np.sin(phi), 0.0]
        np.testing.assert_allclose(extr[i].numpy(), _extr_ref(pos, (0, 0, 2.5)), rtol=0, atol=1e-6)
    np.testing.assert_allclose(stereo_cameras(0.2, 4.0)[1].numpy(), _extr_ref([0.2 * np.cos(np.pi), 0.2 * np.sin(np.pi), 0.0], (0, 0, 4.0)),
                               rtol=0, atol=1e-6)
    assert extr[0, 0, 3] < 0 < extr[1, 0, 3]          # the eyes sit at +x and -x


@pytest.mark.parametrize("W,H", [(96, 64), (854, 480), (64, 96)])
def test_canonical_intrinsics(W, H):
    from splatter_a_video_amd.views import canonical_intrinsics
    k = canonical_intrinsics(W, H)
    fovx = np.pi / 2.0
    focal = W / (2 * np.tan(fovx / 2))
    fovy = 2 * np.arctan(H / (2 * focal))
    want = np.array([W / (2 * np.tan(fovx * 0.5)), H / (2 * np.tan(fovy * 0.5)), W / 2, H / 2], np.float32)
    assert k.dtype == torch.float32 and np.array_equal(k.numpy(), want)
    np.testing.assert_allclose(k.numpy(), [W / 2, W / 2, W / 2, H / 2], rtol=1e-6)     # fovX = pi / 2: the focal length is W / 2


# ------------------------------------------------------------------ the pinned float32 mix against the reference's float64
def test_anaglyph_table():
    from splatter_a_video_amd.views import ANAGLYPH
    assert sorted(ANAGLYPH) == ["color", "halfcolor", "mono", "optimized", "true"]
    for name, m in ANAGLYPH.items():
        m = np.array(m)
        assert m.shape == (3, 6) and (m >= 0).all() and (m.sum(1) <= 1.0 + 1e-12).all(), name
        assert (m[0, 3:] == 0).all() and (m[1:, :3] == 0).all(), name          # red from the left eye, green / blue from the right
    assert ANAGLYPH["optimized"][0] == (0.0, 0.7, 0.3, 0.0, 0.0, 0.0)
    assert ANAGLYPH["true"][1] == (0.0,) * 6


@pytest.mark.parametrize("name", ["true", "mono", "color", "halfcolor", "optimized"])
def test_float32_mix_is_the_float64_formula_up_to_truncation_ties(name):
    """float32 rounding moves o_c * 255 by about 1e-5 of a level, so the truncated bytes differ only where the float64 value
    sits within that of an integer (saturated inputs make such ties: luma weights that sum to 1 in one precision and to
    1 - 2^-24 in the other): by one level at most"""
    from splatter_a_video_amd.views import ANAGLYPH
    rng = np.random.default_rng(11)
    left = rng.uniform(-0.2, 1.2, size=(2, 3, 37, 29)).astype(np.float32)
    right = rng.uniform(-0.2, 1.2, size=(2, 3, 37, 29)).astype(np.float32)
    left[0, :, 0, :8] = (np.arange(8, dtype=np.float32) * 32 / 255)[None]          # exact levels: the ties
    right[0, :, 0, :8] = (np.arange(8, dtype=np.float32) * 32 / 255)[None]
    a = VR.anaglyph(left, right, np.array(ANAGLYPH[name], np.float32))
    b = VR.anaglyph_f64(left, right, np.array(ANAGLYPH[name], np.float64))
    assert a.shape == b.shape == (2, 37, 29, 3) and a.dtype == np.uint8
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    assert d.max() <= 1


def test_to_uint8_restatement():
    x = np.array([-1.0, 0.0, 0.5, 1.0, 2.0, np.nan, 17 / 255, np.inf, -np.inf], np.float32).reshape(1, 3, 1, 3)
    want = np.array([0, 0, 127, 255, 255, 0, int(np.float32(17 / 255) * np.float32(255)), 255, 0], np.uint8).reshape(1, 3, 1, 3)
    assert np.array_equal(VR.to_uint8(x), want.transpose(0, 2, 3, 1))
