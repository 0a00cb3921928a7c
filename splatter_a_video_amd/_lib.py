"""ctypes binding of libsplat_hip.so (C ABI: include/splat_hip.h and its extensions include/splat_hip_views.h,
include/splat_hip_views_grad.h, include/splat_hip_camera_grad.h, include/splat_hip_layers_cam.h, include/splat_hip_flow.h and
include/splat_hip_flow_occ.h).

The product path has NO fallback: if the HIP library is missing or a tensor is not a contiguous
float32/int32 CUDA tensor the call raises.  (The CPU oracle lives in ``oracle/`` and is never
imported from here.)
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPLAT_LIB_PATH: another build of the same ABI to load instead; default = in-tree library
LIB_PATH = os.environ.get("SPLAT_LIB_PATH") or os.path.join(_HERE, "libsplat_hip.so")
_lib: Optional[ctypes.CDLL] = None


def _load(file: str, base=None):
    return _abi.load(os.path.join(_HERE, os.pardir, "include", file), base)


# the header is the only place a prototype, a struct or a constant of the ABI is written (_abi.py reads it)
CORE = ("splat_hip.h", "SPLAT_ABI_VERSION", "splat_abi_version")
HEADER = _load(CORE[0])
ABI_VERSION = HEADER.defines[CORE[1]]
MAX_SOURCES = HEADER.defines["SPLAT_MAX_SOURCES"]
SYMBOLS = list(HEADER.functions)
FeatureSource = HEADER.structs["splat_feature_source_t"]
# entry points added after the core header was frozen: a header of their own (it includes the core header for its handles and
# structs and brings none of its own: the names its prototypes use are the core header's), the same library, a version of their
# own.  One row per extension: (file name, version define, version function) -- the cameras per frame and the pinhole camera of a
# dynamic batch; training under those cameras; the camera gradients of a dynamic batch; layered scenes (layer editing, feature
# lifting) under those cameras; dense optical flow (the flow attribute of frame pairs, flow colours, flow error)
EXTENSIONS = (("splat_hip_views.h", "SPLAT_VIEWS_ABI_VERSION", "splat_views_abi_version"),
              ("splat_hip_views_grad.h", "SPLAT_VIEWS_GRAD_ABI_VERSION", "splat_views_grad_abi_version"),
              ("splat_hip_camera_grad.h", "SPLAT_CAMERA_GRAD_ABI_VERSION", "splat_camera_grad_abi_version"),
              ("splat_hip_layers_cam.h", "SPLAT_LAYERS_CAM_ABI_VERSION", "splat_layers_cam_abi_version"),
              ("splat_hip_flow.h", "SPLAT_FLOW_ABI_VERSION", "splat_flow_abi_version"))
_EXT = tuple(_load(file, HEADER) for file, _, _ in EXTENSIONS)
VIEWS_HEADER, VIEWS_GRAD_HEADER, CAMERA_GRAD_HEADER, LAYERS_CAM_HEADER, FLOW_HEADER = _EXT
VIEWS_ABI_VERSION, VIEWS_GRAD_ABI_VERSION, CAMERA_GRAD_ABI_VERSION, LAYERS_CAM_ABI_VERSION, FLOW_ABI_VERSION = (
    h.defines[define] for h, (_, define, _) in zip(_EXT, EXTENSIONS))
VIEWS_SYMBOLS, VIEWS_GRAD_SYMBOLS, CAMERA_GRAD_SYMBOLS, LAYERS_CAM_SYMBOLS, FLOW_SYMBOLS = (list(h.functions) for h in _EXT)
# extension headers after those five (EXTENSIONS keeps its rows): where a dense flow is valid -- the flow attribute with the
# depth, occlusion masks and warped frames
LATER_EXTENSIONS = (("splat_hip_flow_occ.h", "SPLAT_FLOW_OCC_ABI_VERSION", "splat_flow_occ_abi_version"),)
_LATER = tuple(_load(file, HEADER) for file, _, _ in LATER_EXTENSIONS)
FLOW_OCC_HEADER, = _LATER
FLOW_OCC_ABI_VERSION = FLOW_OCC_HEADER.defines[LATER_EXTENSIONS[0][1]]
FLOW_OCC_SYMBOLS = list(FLOW_OCC_HEADER.functions)


class SplatError(RuntimeError):
    pass


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SplatError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C splatter_a_video_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        headers = ((CORE, HEADER),) + tuple(zip(EXTENSIONS, _EXT)) + tuple(zip(LATER_EXTENSIONS, _LATER))
        for (file, _, _), h in headers:
            for name, (restype, argtypes) in h.functions.items():
                fn = getattr(L, name, None)
                if fn is None:
                    raise SplatError(f"{LIB_PATH} lacks {name} (include/{file}: the library is older than the headers); rebuild it")
                fn.restype, fn.argtypes = restype, argtypes
        for (file, define, version), h in headers:
            have = getattr(L, version)()
            if have != h.defines[define]:
                kind = "-".join(define.split("_")[1:-2]).lower()      # "", "views", "views-grad", ...
                raise SplatError(f"{LIB_PATH} has {kind + ' ' if kind else ''}ABI version {have}, include/{file} "
                                 f"{h.defines[define]}; rebuild it")
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise SplatError(f"libsplat_hip error {rc}: {lib().splat_last_error().decode()}")


def ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def stream() -> ctypes.c_void_p:
    """the current HIP stream of the current device (raw handle).  torch.cuda.current_stream() builds a Stream object
    through several Python layers (~10 us per call, once per native launch); the raw getter is one C call."""
    if _raw_stream is not None and _cur_device is not None:
        return ctypes.c_void_p(_raw_stream(_cur_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# cf / ci: explicit scalar wrappers from before every function had argtypes.  The package passes plain Python values;
# the two stay for callers outside it (bench.py, scripts and tests written against the earlier binding)
def cf(x: float) -> ctypes.c_float:
    return ctypes.c_float(float(x))


def ci(x: int) -> ctypes.c_int:
    return ctypes.c_int(int(x))


def need(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    """Device / dtype gate + contiguity (the reference calls .contiguous() on every input too)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA (ROCm) tensor")
    if _cur_device is not None and t.device.index != _cur_device():
        # kernels are launched on the CURRENT device's stream (stream() below): a tensor of another device would be
        # dereferenced there.  One process drives one GPU (frame-sharded DP); otherwise wrap the call in torch.cuda.device(...)
        raise ValueError(f"{name} lives on cuda:{t.device.index} but the current device is cuda:{_cur_device()}")
    if t.dtype != dtype:
        if dtype == torch.uint8 and t.dtype == torch.bool:
            t = t.contiguous().view(torch.uint8)
        else:
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def build_id() -> str:
    """hash of the sources the loaded library was built from (csrc/Makefile); measurement records carry it"""
    return lib().splat_build_id().decode()


def set_option(key: str, value: int) -> None:
    """process-wide option of the library (include/splat_hip.h: splat_set_option): "bwd_quarters", "sets_std", "bin_slot_keys",
    "bin_short_segments", "deterministic"; read at launch time"""
    check(lib().splat_set_option(key.encode(), int(value)))


def get_option(key: str) -> int:
    v = ctypes.c_int(0)
    check(lib().splat_get_option(key.encode(), ctypes.byref(v)))
    return v.value


class option:
    """``with L.option("bwd_quarters", 0): ...`` -- an option for the duration of a block (tests)"""

    def __init__(self, key: str, value: int):
        self.key, self.value = key, int(value)

    def __enter__(self):
        self.old = get_option(self.key)
        set_option(self.key, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.key, self.old)
        return False


def set_deterministic(on: bool) -> None:
    """process-wide deterministic mode (include/splat_hip.h: splat_set_deterministic): no backward launches a kernel with
    float atomics; a foreign idx_sorted (atomic backward) raises"""
    lib().splat_set_deterministic(1 if on else 0)


def deterministic() -> bool:
    return bool(lib().splat_get_deterministic())


def profile_enable(on: bool) -> None:
    lib().splat_profile_enable(1 if on else 0)


def profile_reset() -> None:
    lib().splat_profile_reset()


def profile_read(prefix: str = ""):
    ms = ctypes.c_double(0.0)
    n = ctypes.c_int(0)
    lib().splat_profile_read(prefix.encode(), ctypes.byref(ms), ctypes.byref(n))
    return ms.value, n.value
