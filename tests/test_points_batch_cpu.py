"""The frame-batched sparse compositing and the per-query track loss without a GPU: splat_alpha_blending_points_forward_batch /
_backward_batch (csrc/query.hip) and splat_track_loss_grad_points (csrc/loss.hip) exported, declared, listed and refusing bad
arguments with SPLAT_E_ARG before any HIP call; additions only, so the ABI version stays 22."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FWD = "splat_alpha_blending_points_forward_batch"
BWD = "splat_alpha_blending_points_backward_batch"
LOSS = "splat_track_loss_grad_points"
ONE = ctypes.c_void_p(16)          # never dereferenced: every call of these tests is refused or returns on the host
I64, F32 = ctypes.c_int64, ctypes.c_float


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_symbols_are_exported_declared_listed_and_the_abi_version_stays(L):
    so = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    declared = set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", header))
    for name in (FWD, BWD, LOSS):
        assert name in L.SYMBOLS and hasattr(so, name) and name in declared, name
    lib = L.lib()
    assert len(lib.splat_alpha_blending_points_forward_batch.argtypes) == 22
    assert len(lib.splat_alpha_blending_points_backward_batch.argtypes) == 28
    assert len(lib.splat_track_loss_grad_points.argtypes) == 18
    assert lib.splat_abi_version() == 22 and L.ABI_VERSION == 22
    assert re.search(r"#define SPLAT_ABI_VERSION 22\b", header)
    # what the backward relies on, and its determinism rule, are part of the entry's contract
    doc = header[header.index(BWD + ":"):][:2500]
    assert "RELIES ON" in doc and "splat_set_deterministic(1)" in doc and "SPLAT_E_ARG" in doc
    # the record fields live in one place
    common = open(os.path.join(ROOT, "splatter_a_video_amd", "csrc", "common.h")).read()
    assert re.search(r"REC_UX = 0, REC_UY = 1, REC_CA = 2, REC_CB = 3, REC_CC = 4, REC_O = 5", common)


def _fwd(lib, **k):
    a = dict(F=3, P=10, C=3, uv=ONE, conic=ONE, op=ONE, ofs=0, feat=ONE, ffs=0, idx=ONE, tr=ONE, cap=100, bg=0.0, W=64, H=48, Q=5,
             off=ONE, pts=ONE, out=ONE, cT=ONE, cn=ONE)
    a.update(k)
    return lib.splat_alpha_blending_points_forward_batch(
        a["F"], a["P"], a["C"], a["uv"], a["conic"], a["op"], I64(a["ofs"]), a["feat"], I64(a["ffs"]), a["idx"], a["tr"],
        I64(a["cap"]), F32(a["bg"]), a["W"], a["H"], I64(a["Q"]), a["off"], a["pts"], a["out"], a["cT"], a["cn"], None)


def _bwd(lib, **k):
    a = dict(F=3, P=10, C=3, uv=ONE, conic=ONE, op=ONE, ofs=0, feat=ONE, ffs=0, idx=ONE, tr=ONE, cap=100, bg=0.0, W=64, H=48, Q=5,
             off=ONE, pts=ONE, cT=ONE, cn=ONE, g=ONE, slot=ONE, rec=ONE, rs=16, detach=1, dfeat=ONE, dfs=0)
    a.update(k)
    return lib.splat_alpha_blending_points_backward_batch(
        a["F"], a["P"], a["C"], a["uv"], a["conic"], a["op"], I64(a["ofs"]), a["feat"], I64(a["ffs"]), a["idx"], a["tr"],
        I64(a["cap"]), F32(a["bg"]), a["W"], a["H"], I64(a["Q"]), a["off"], a["pts"], a["cT"], a["cn"], a["g"], a["slot"],
        a["rec"], a["rs"], a["detach"], a["dfeat"], I64(a["dfs"]), None)


def _loss(lib, **k):
    a = dict(F=3, H=48, W=64, C=3, vals=ONE, off=ONE, pix=ONE, tgt=ONE, Q=5, fw=ONE, q=0.98, scale=1.0, grad=ONE, pf=ONE, slot=ONE,
             counts=ONE, scratch=ONE)
    a.update(k)
    return lib.splat_track_loss_grad_points(a["F"], a["H"], a["W"], a["C"], a["vals"], a["off"], a["pix"], a["tgt"], I64(a["Q"]),
                                            a["fw"], F32(a["q"]), F32(a["scale"]), a["grad"], a["pf"], a["slot"], a["counts"],
                                            a["scratch"], None)


def test_forward_batch_validates_before_hip(L):
    lib = L.lib()
    assert _fwd(lib, F=0) == -1 and b"sizes" in lib.splat_last_error() and FWD.encode() in lib.splat_last_error()
    for bad in (dict(P=-1), dict(C=0), dict(W=0), dict(H=-2), dict(Q=-1), dict(cap=-1), dict(ofs=-1), dict(ffs=-1)):
        assert _fwd(lib, **bad) == -1 and b"sizes" in lib.splat_last_error(), bad
    assert _fwd(lib, W=(1 << 24) + 1) == -1 and b"too large" in lib.splat_last_error()
    assert _fwd(lib, Q=1 << 31) == -1 and b"too large" in lib.splat_last_error()
    for k in ("pts", "out", "off", "uv", "conic", "op", "feat", "tr"):
        assert _fwd(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k


def test_backward_batch_validates_before_hip(L):
    lib = L.lib()
    assert _bwd(lib, F=0) == -1 and b"sizes" in lib.splat_last_error() and BWD.encode() in lib.splat_last_error()
    for bad in (dict(P=-1), dict(C=0), dict(W=0), dict(H=-2), dict(Q=-1), dict(cap=-1), dict(ofs=-1), dict(ffs=-1), dict(dfs=-1),
                dict(rs=4), dict(rs=18), dict(cap=0)):
        assert _bwd(lib, **bad) == -1 and b"sizes" in lib.splat_last_error(), bad
    assert _bwd(lib, H=(1 << 24) + 1) == -1 and b"too large" in lib.splat_last_error()
    for k in ("pts", "off", "cT", "cn", "g", "uv", "conic", "op", "feat", "tr", "slot", "idx"):
        assert _bwd(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k


def test_loss_entry_validates_before_hip(L):
    lib = L.lib()
    assert _loss(lib, F=0) == -1 and b"sizes" in lib.splat_last_error() and LOSS.encode() in lib.splat_last_error()
    for bad in (dict(H=0), dict(W=0), dict(C=1), dict(Q=-1)):
        assert _loss(lib, **bad) == -1 and b"sizes" in lib.splat_last_error(), bad
    assert _loss(lib, Q=1 << 31) == -1 and b"too large" in lib.splat_last_error()
    assert _loss(lib, q=1.5) == -1 and b"quantile" in lib.splat_last_error()
    for k in ("off", "fw", "scratch", "vals", "pix", "tgt"):
        assert _loss(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k
    assert _loss(lib, tgt=ctypes.c_void_p(20)) == -1 and b"aligned" in lib.splat_last_error()


def test_nothing_to_do_is_valid_without_any_pointer(L):
    lib = L.lib()
    none = dict(uv=None, conic=None, op=None, feat=None, idx=None, tr=None, off=None, pts=None, cT=None, cn=None)
    assert _fwd(lib, Q=0, out=None, **none) == 0
    assert _fwd(lib, Q=0, P=0, out=None, **none) == 0
    back = dict(none, g=None, slot=None, rec=None, dfeat=None)
    assert _bwd(lib, Q=0, **back) == 0
    assert _bwd(lib, Q=0, P=0, **back) == 0
    # no Gaussians: nothing to add to, the Gaussian-side pointers may be NULL
    assert _bwd(lib, P=0, uv=None, conic=None, op=None, feat=None, idx=None, tr=None, slot=None, rec=None, dfeat=None) == 0
    # no output wanted: nothing is launched
    assert _bwd(lib, slot=None, rec=None, dfeat=None) == 0


def test_python_layers_refuse_what_they_cannot_serve(L):
    import torch
    from splatter_a_video_amd import losses
    from splatter_a_video_amd.frames import _parse_points
    from splatter_a_video_amd.tracks import TrackTargets
    tt = TrackTargets.from_reference([[1.0, 1.0], [2.0, 1.0]], [[0.0, 0.0, -9.0, -9.0]] * 2, 8, 8)
    with pytest.raises(ValueError, match="CUDA"):
        losses.track_loss_points_grad(torch.zeros(2, 3), tt, torch.ones(1))          # no CPU fallback
    assert _parse_points(None, None, 2, 4) is None
    with pytest.raises(ValueError, match="feature"):
        _parse_points(dict(feature=torch.zeros(4, 3), points=torch.zeros(1, 2), offsets=torch.zeros(3, dtype=torch.int64)), None, 2, 4)
    with pytest.raises(ValueError, match="unknown"):
        _parse_points(dict(feature=torch.zeros(4, 3), colour=1), None, 2, 4)
