"""The wide detached set of the frame batch without a GPU: splat_alpha_blending_forward_batch_set, its backward twin
splat_alpha_blending_backward_batch_set_packed (csrc/blend.hip) and splat_frames_wide_fold (csrc/frames.hip) exported, declared,
listed and refusing bad arguments with SPLAT_E_ARG before any HIP call; additions only, so the ABI version stays 22; and the
validation of ``wide=`` in frames.py."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FWD = "splat_alpha_blending_forward_batch_set"
BWD = "splat_alpha_blending_backward_batch_set_packed"
FOLD = "splat_frames_wide_fold"
ONE = ctypes.c_void_p(16)          # never dereferenced: every call of these tests is refused on the host
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
    for name in (FWD, BWD, FOLD):
        assert name in L.SYMBOLS and hasattr(so, name) and name in declared, name
    lib = L.lib()
    assert len(lib.splat_alpha_blending_forward_batch_set.argtypes) == 23
    assert len(lib.splat_alpha_blending_backward_batch_set_packed.argtypes) == 20
    assert len(lib.splat_frames_wide_fold.argtypes) == 12
    assert lib.splat_abi_version() == 22 and L.ABI_VERSION == 22
    assert re.search(r"#define SPLAT_ABI_VERSION 22\b", header)
    # the fold's contract: what it leaves out, and that it needs no atomics
    doc = header[header.index("splat_frames_wide_fold, ONE"):][:1500]
    assert "`o` is left out" in doc and "No float atomics" in doc


def _fwd(lib, **k):
    a = dict(F=3, P=10, C=70, c0=32, cn=32, uv=ONE, conic=ONE, op=ONE, ofs=0, feat=ONE, ffs=0, idx=ONE, tr=ONE, cap=100, bg=0.0,
             W=64, H=48, out=ONE, fT=ONE, nc=ONE, pack=ONE, cull=None)
    a.update(k)
    return lib.splat_alpha_blending_forward_batch_set(
        a["F"], a["P"], a["C"], a["c0"], a["cn"], a["uv"], a["conic"], a["op"], I64(a["ofs"]), a["feat"], I64(a["ffs"]), a["idx"],
        a["tr"], I64(a["cap"]), F32(a["bg"]), a["W"], a["H"], a["out"], a["fT"], a["nc"], a["pack"], a["cull"], None)


def _bwd(lib, **k):
    a = dict(F=3, P=10, C=70, c0=64, cn=6, idx=ONE, tr=ONE, cap=100, bg=0.0, W=64, H=48, fT=ONE, nc=ONE, g=ONE, slot=ONE, rec=ONE,
             pack=ONE, cull=ONE, dbg=None)
    a.update(k)
    return lib.splat_alpha_blending_backward_batch_set_packed(
        a["F"], a["P"], a["C"], a["c0"], a["cn"], a["idx"], a["tr"], I64(a["cap"]), F32(a["bg"]), a["W"], a["H"], a["fT"], a["nc"],
        a["g"], a["slot"], a["rec"], a["pack"], a["cull"], a["dbg"], None)


def _fold(lib, **k):
    a = dict(F=3, P=10, cn=32, cap=100, goff=ONE, tail=ONE, row=ONE, rs=20, dfeat=ONE, dfs=70, c0=32)
    a.update(k)
    return lib.splat_frames_wide_fold(a["F"], a["P"], a["cn"], I64(a["cap"]), a["goff"], a["tail"], a["row"], a["rs"], a["dfeat"],
                                      I64(a["dfs"]), a["c0"], None)


def test_forward_chunk_validates_before_hip(L):
    lib = L.lib()
    assert _fwd(lib, F=0) == -1 and b"sizes" in lib.splat_last_error() and FWD.encode() in lib.splat_last_error()
    for bad in (dict(P=0), dict(C=0), dict(W=0), dict(H=-2), dict(cap=0), dict(ofs=-1), dict(ffs=-1)):
        assert _fwd(lib, **bad) == -1 and b"sizes" in lib.splat_last_error(), bad
    for bad in (dict(c0=-1), dict(cn=0), dict(cn=33), dict(c0=64, cn=7), dict(C=40, c0=32, cn=9)):
        assert _fwd(lib, **bad) == -1 and b"chunk" in lib.splat_last_error(), bad
    for k in ("uv", "conic", "op", "feat", "idx", "tr", "out", "fT", "nc", "pack"):
        assert _fwd(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k
    assert _fwd(lib, W=1 << 16, H=1 << 16, F=1 << 10) == -1 and b"too many tiles" in lib.splat_last_error()


def test_backward_chunk_validates_before_hip(L):
    lib = L.lib()
    assert _bwd(lib, F=0) == -1 and b"sizes" in lib.splat_last_error() and BWD.encode() in lib.splat_last_error()
    for bad in (dict(P=0), dict(C=0), dict(W=0), dict(H=-2), dict(cap=0)):
        assert _bwd(lib, **bad) == -1 and b"sizes" in lib.splat_last_error(), bad
    for bad in (dict(c0=-1), dict(cn=0), dict(cn=33, c0=0), dict(c0=64, cn=7)):
        assert _bwd(lib, **bad) == -1 and b"chunk" in lib.splat_last_error(), bad
    for k in ("idx", "tr", "fT", "nc", "g", "slot", "rec", "pack"):
        assert _bwd(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k
    assert _bwd(lib, W=1 << 16, H=1 << 16, F=1 << 10) == -1 and b"too many tiles" in lib.splat_last_error()


def test_every_frame_batch_backward_refuses_too_many_tiles(L):
    """F * tiles must fit an int in every frame-batch entry of csrc/blend.hip: the row's, the set's and the three-set backward
    refuse the shape their forward refuses (the chunk's twin is checked above)"""
    lib = L.lib()
    F, W, H = 1 << 10, 1 << 16, 1 << 16

    def i3(*v):
        return (ctypes.c_int32 * 3)(*v)

    assert lib.splat_alpha_blending_backward_batch(F, 10, 3, ONE, ONE, 100, 0.0, W, H, ONE, ONE, ONE, 0, ONE, ONE, ONE, ONE, None, None) == -1
    assert lib.splat_last_error() == b"splat_alpha_blending_backward_batch: too many tiles"
    assert lib.splat_alpha_blending_backward_batch_set(F, 10, 23, 4, 19, ONE, ONE, ONE, 0, ONE, 0, ONE, ONE, 100, 0.0, W, H, ONE, ONE, ONE,
                                                       0, ONE, ONE, ONE, None, None) == -1
    assert lib.splat_last_error() == b"splat_alpha_blending_backward_batch_set: too many tiles"
    assert lib.splat_alpha_blending_backward_batch_sets(F, 10, 23, i3(0, 3, 4), i3(3, 1, 19), (F32 * 3)(0.2, 1.0, 0.0), ONE, ONE, ONE, 0,
                                                        ONE, 0, None, None, ONE, ONE, 100, W, H, ONE, ONE, ONE, None, 0, ONE, ONE, ONE,
                                                        ONE, None, None) == -1
    assert lib.splat_last_error().endswith(b": too many tiles")


def test_fold_validates_before_hip(L):
    lib = L.lib()
    assert _fold(lib, F=0) == -1 and b"sizes" in lib.splat_last_error() and FOLD.encode() in lib.splat_last_error()
    for bad in (dict(P=0), dict(cn=0), dict(cn=33), dict(cap=0), dict(c0=-1), dict(rs=4), dict(rs=18), dict(rs=-8), dict(dfs=63),
                dict(dfs=-1)):
        assert _fold(lib, **bad) == -1 and b"sizes" in lib.splat_last_error(), bad
    for k in ("goff", "tail", "row"):
        assert _fold(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k
    assert _fold(lib, tail=ctypes.c_void_p(20)) == -1 and b"aligned" in lib.splat_last_error()
    assert _fold(lib, row=ctypes.c_void_p(24)) == -1 and b"aligned" in lib.splat_last_error()


def test_wide_validation(L):
    import torch
    from splatter_a_video_amd.frames import _parse_wide
    P = 4
    f = torch.zeros(P, 40)
    assert _parse_wide(None, None, P) is None
    with pytest.raises(ValueError, match="pass wide="):                       # a sink without the set
        _parse_wide(None, torch.zeros(P, 40), P)
    with pytest.raises(ValueError, match="unknown"):
        _parse_wide(dict(feature=f, detach_opacity=True, taps=True), None, P)
    for bad in (dict(feature=f, detach_opacity=False), dict(feature=f), dict(feature=f, detach_opacity=1)):
        with pytest.raises(ValueError, match="detach_opacity must be True"):
            _parse_wide(bad, None, P)
    for shape in ((P + 1, 40), (P, 0), (2, P, 40), (P,)):
        with pytest.raises(ValueError, match=r"\[P=4, c\]"):
            _parse_wide(dict(feature=torch.zeros(*shape), detach_opacity=True), None, P)
    with pytest.raises(ValueError, match=r"\[P=4, c\]"):
        _parse_wide(dict(feature=f.double(), detach_opacity=True), None, P)
    with pytest.raises(ValueError, match="no CPU path"):                      # a well-formed set still needs the GPU
        _parse_wide(dict(feature=f, detach_opacity=True), None, P)
