"""Golden vectors for the flow colours from the reference's own ``util.flow_to_image`` (src/util.py:510-536, with
``make_colorwheel`` and ``flow_uv_to_colors``, :421-507), called on the CPU.  The module's imports this container lacks
(``torchvision``, ``imageio``, ``cv2``) are stubbed; none of them is used by these functions.  Inputs and bytes only: data travels.

    python tests/golden/make_golden_flow.py    ->  tests/golden/flow_wheel.npz

Cases (``<case>_flow`` float32 [..., H, W, 2] as the reference takes it, ``<case>_img`` uint8): ``random`` (48 x 64, normal,
sigma = 3 px), ``odd`` (37 x 53), ``zeros`` (white), ``directions`` (the eight axis and diagonal directions at three radii),
``stack`` (a 4-D stack of 3 frames: one maximum for all), ``clip`` (``clip_flow = 2.5``), ``bgr`` (``convert_to_bgr``); and
``wheel``, the 55 x 3 table of ``make_colorwheel``.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))
CLIP_FLOW = 2.5


def _stubs():
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    for name in ("imageio", "cv2"):
        sys.modules[name] = types.ModuleType(name)


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def cases():
    rng = np.random.default_rng(20240607)
    f = lambda *s: rng.normal(0, 3.0, size=s).astype(np.float32)
    out = {"random": (f(48, 64, 2), {}), "odd": (f(37, 53, 2), {}), "zeros": (np.zeros((16, 24, 2), np.float32), {})}
    d = np.zeros((3, 8, 2), np.float32)
    for r, rad in enumerate((0.5, 2.0, 4.0)):
        for k in range(8):
            a = k * np.pi / 4
            d[r, k] = rad * np.round(np.array([np.cos(a), np.sin(a)])).astype(np.float32)
    out["directions"] = (d, {})
    out["stack"] = (f(3, 20, 28, 2) * np.array([0.3, 1.0, 2.0], np.float32)[:, None, None, None], {})
    out["clip"] = (f(30, 40, 2), dict(clip_flow=CLIP_FLOW))
    out["bgr"] = (f(24, 32, 2), dict(convert_to_bgr=True))
    return out


def main():
    _stubs()
    util = _load("ref_util", "util.py")
    data = {"wheel": util.make_colorwheel().astype(np.float64), "numpy_version": np.array(np.__version__)}
    for name, (flow, kw) in cases().items():
        img = util.flow_to_image(flow.copy(), **kw)
        assert img.dtype == np.uint8 and img.shape == flow.shape[:-1] + (3,)
        data[name + "_flow"], data[name + "_img"] = flow, img
    np.savez_compressed(os.path.join(HERE, "flow_wheel.npz"), **data)
    print({k: v.shape for k, v in data.items()})


if __name__ == "__main__":
    main()
