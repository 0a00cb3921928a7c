"""The backward of the sparse compositing without a GPU: splat_alpha_blending_points_backward (csrc/query.hip) exported, declared
and refusing bad arguments with SPLAT_E_ARG before any HIP call, and gs.alpha_blending_points(differentiable=True) refusing what
it cannot serve while the default stays forward only."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAME = "splat_alpha_blending_points_backward"
LIVE = "splat_alpha_blending_points_forward_live"       # its forward: corners without weight are not walked


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_symbol_is_exported_declared_listed_and_the_abi_version_stays(L):
    so = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    declared = set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", header))
    for name in (NAME, LIVE):
        assert name in L.SYMBOLS and hasattr(so, name) and name in declared, name
    assert len(L.lib().splat_alpha_blending_points_backward.argtypes) == 21
    assert L.lib().splat_abi_version() == 22 and L.ABI_VERSION == 22
    assert re.search(r"#define SPLAT_ABI_VERSION 22\b", header)
    # the determinism rule is part of the entry's contract
    doc = header[header.index("splat_alpha_blending_points_backward:"):]
    assert "splat_set_deterministic(1)" in doc[:2500] and "SPLAT_E_ARG" in doc[:2500]


def _call(lib, **k):
    one = ctypes.c_void_p(16)          # never dereferenced: every call of these tests is refused or returns on the host
    a = dict(P=10, C=3, uv=one, conic=one, op=one, feat=one, idx=one, tr=one, bg=0.0, W=64, H=48, Q=5, pts=one, cT=one, cn=one,
             g=one, duv=one, dconic=one, dop=one, dfeat=one)
    a.update(k)
    return lib.splat_alpha_blending_points_backward(a["P"], a["C"], a["uv"], a["conic"], a["op"], a["feat"], a["idx"], a["tr"],
                                                    a["bg"], a["W"], a["H"], a["Q"], a["pts"], a["cT"], a["cn"],
                                                    a["g"], a["duv"], a["dconic"], a["dop"], a["dfeat"], None)


def test_backward_entry_validates_before_hip(L):
    lib = L.lib()
    assert _call(lib, P=-1) == -1 and b"sizes" in lib.splat_last_error()
    assert b"splat_alpha_blending_points_backward" in lib.splat_last_error()
    assert _call(lib, C=0) == -1 and _call(lib, W=0) == -1 and _call(lib, H=-2) == -1 and _call(lib, Q=-1) == -1
    assert _call(lib, W=(1 << 24) + 1) == -1 and b"too large" in lib.splat_last_error()
    assert _call(lib, H=(1 << 24) + 1) == -1 and b"too large" in lib.splat_last_error()
    assert _call(lib, pts=None) == -1 and b"null" in lib.splat_last_error()
    for k in ("cT", "cn", "g"):
        assert _call(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k
    for k in ("uv", "conic", "op", "feat", "tr"):
        assert _call(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k


def test_live_forward_entry_validates_like_the_forward(L):
    lib = L.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: every call below is refused on the host
    f = ctypes.c_float

    def call(P=10, C=3, uv=one, conic=one, op=one, feat=one, idx=one, tr=one, bg=0.0, W=64, H=48, Q=5, pts=one, out=one):
        return lib.splat_alpha_blending_points_forward_live(P, C, uv, conic, op, feat, idx, tr, f(bg), W, H, Q, pts, out, None, None, None)
    assert call(P=-1) == -1 and b"sizes" in lib.splat_last_error()
    assert call(C=0) == -1 and call(W=0) == -1 and call(H=-2) == -1 and call(Q=-1) == -1
    assert call(W=(1 << 24) + 1) == -1 and b"too large" in lib.splat_last_error()
    assert call(pts=None) == -1 and b"null" in lib.splat_last_error()
    assert call(out=None) == -1
    assert call(uv=None) == -1 and call(conic=None) == -1 and call(op=None) == -1 and call(feat=None) == -1 and call(tr=None) == -1
    assert call(Q=0, pts=None, out=None, uv=None, conic=None, op=None, feat=None, idx=None, tr=None) == 0


def test_nothing_to_do_is_valid_without_any_pointer(L):
    lib = L.lib()
    none = dict(uv=None, conic=None, op=None, feat=None, idx=None, tr=None, pts=None, cT=None, cn=None, g=None, duv=None,
                dconic=None, dop=None, dfeat=None)
    assert _call(lib, Q=0, **none) == 0
    assert _call(lib, Q=0, P=0, **none) == 0
    # no Gaussians: nothing to add to, the Gaussian-side pointers may be NULL
    assert _call(lib, P=0, uv=None, conic=None, op=None, feat=None, idx=None, tr=None, duv=None, dconic=None, dop=None, dfeat=None) == 0
    # every output NULL: nothing is launched
    assert _call(lib, duv=None, dconic=None, dop=None, dfeat=None) == 0


def test_python_operator_refuses_what_it_cannot_serve(L):
    import dptr.gs as gs
    from splatter_a_video_amd import gs as native
    from splatter_a_video_amd import losses
    assert gs.alpha_blending_points is native.alpha_blending_points
    assert callable(losses.track_loss_sparse)
    z = lambda *s, **k: torch.zeros(*s, **k)
    args = lambda **k: dict(dict(uv=z(4, 2), conic=z(4, 3), opacity=z(4, 1), feature=z(4, 3), idx_sorted=z(0, dtype=torch.int32),
                                 tile_range=z(4, 2, dtype=torch.int32), bg=0.0, W=32, H=32, points=z(5, 2)), **k)
    with pytest.raises(ValueError, match="CUDA"):
        gs.alpha_blending_points(**args(), differentiable=True)                    # no CPU fallback
    with pytest.raises(ValueError, match="CUDA"):
        gs.alpha_blending_points(**args(feature=z(4, 3, requires_grad=True)), differentiable=True)
    with pytest.raises(ValueError, match="points"):
        gs.alpha_blending_points(**args(points=z(5, 2, requires_grad=True)), differentiable=True)
    # the default is what it was: forward only
    with pytest.raises(ValueError, match="forward only"):
        gs.alpha_blending_points(**args(feature=z(4, 3, requires_grad=True)))
    with pytest.raises(ValueError, match="forward only"):
        gs.alpha_blending_points(**args(uv=z(4, 2, requires_grad=True)), differentiable=False)
