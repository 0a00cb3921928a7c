"""The ordered (float-atomic-free) backward of the sparse compositing without a GPU: splat_alpha_blending_points_backward_ordered /
_batch_ordered and their scratch-size queries (csrc/query.hip) exported, declared, listed, sized as the header documents and
refusing bad arguments with SPLAT_E_ARG before any HIP call; additions only, so the ABI version stays 22."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ONE_ = "splat_alpha_blending_points_backward_ordered"
BATCH = "splat_alpha_blending_points_backward_batch_ordered"
NEW = [ONE_, ONE_ + "_scratch_bytes", BATCH, BATCH + "_scratch_bytes"]
ONE = ctypes.c_void_p(16)          # never dereferenced: every call of these tests is refused or returns on the host
I64, F32, SZ = ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
BIG = 1 << 40


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_symbols_are_exported_declared_listed_and_the_abi_version_stays(L):
    so = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    declared = set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(so, name) and name in declared, name
    lib = L.lib()
    assert len(getattr(lib, ONE_).argtypes) == 26 and len(getattr(lib, BATCH).argtypes) == 31
    assert lib.splat_abi_version() == 22 and L.ABI_VERSION == 22
    assert re.search(r"#define SPLAT_ABI_VERSION 22\b", header)
    # the order of the sums is part of the contract
    doc = header[header.index(ONE_ + " / _batch_ordered"):][:4000]
    for words in ("THE ORDER", "ascending", "slots", "frames ascending", "scratch", "SPLAT_E_ARG"):
        assert words in doc, words


def _documented(NT, Q, records):
    return 16 * ((2 * NT + 1 + 12 * Q + 3) // 4) + 4 * records


def test_scratch_sizes_are_the_documented_ones(L):
    lib = L.lib()
    one, batch = getattr(lib, ONE_ + "_scratch_bytes"), getattr(lib, BATCH + "_scratch_bytes")
    r4 = lambda n: (n + 3) // 4 * 4
    for C, W, H, Q, cap in [(3, 100, 60, 57, 1234), (1, 16, 16, 0, 0), (300, 854, 480, 1000, 70000), (5, 17, 33, 1, 1)]:
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        assert one(C, W, H, Q, cap) == _documented(tiles, Q, cap * r4(6 + C)), (C, W, H, Q, cap)
        for F in (1, 3, 25):
            assert batch(F, C, W, H, Q, cap) == _documented(F * tiles, Q, F * cap * r4(C)), (F, C, W, H, Q, cap)
    for bad in [(0, 64, 48, 5, 10), (3, 0, 48, 5, 10), (3, 64, 0, 5, 10), (3, 64, 48, -1, 10), (3, 64, 48, 5, -1),
                (3, (1 << 24) + 1, 48, 5, 10), (3, 64, 48, (1 << 29) + 1, 10)]:
        assert one(*bad) == 0, bad
        assert batch(2, *bad) == 0, bad
    assert batch(0, 3, 64, 48, 5, 10) == 0 and batch((1 << 16) + 1, 3, 64, 48, 5, 10) == 0


def _one(lib, **k):
    a = dict(P=10, C=3, uv=ONE, conic=ONE, op=ONE, feat=ONE, idx=ONE, tr=ONE, cap=100, bg=0.0, W=64, H=48, Q=5, pts=ONE, cT=ONE,
             cn=ONE, g=ONE, duv=ONE, dconic=ONE, dop=ONE, dfeat=ONE, goff=ONE, slot=ONE, scratch=ONE, nbytes=BIG)
    a.update(k)
    return getattr(lib, ONE_)(a["P"], a["C"], a["uv"], a["conic"], a["op"], a["feat"], a["idx"], a["tr"], I64(a["cap"]), F32(a["bg"]),
                              a["W"], a["H"], a["Q"], a["pts"], a["cT"], a["cn"], a["g"], a["duv"], a["dconic"], a["dop"], a["dfeat"],
                              a["goff"], a["slot"], a["scratch"], SZ(a["nbytes"]), None)


def _batch(lib, **k):
    a = dict(F=3, P=10, C=3, uv=ONE, conic=ONE, op=ONE, ofs=0, feat=ONE, ffs=0, idx=ONE, tr=ONE, cap=100, bg=0.0, W=64, H=48, Q=5,
             off=ONE, pts=ONE, cT=ONE, cn=ONE, g=ONE, slot=ONE, rec=ONE, rs=16, detach=1, dfeat=ONE, dfs=0, goff=ONE, scratch=ONE,
             nbytes=BIG)
    a.update(k)
    return getattr(lib, BATCH)(
        a["F"], a["P"], a["C"], a["uv"], a["conic"], a["op"], I64(a["ofs"]), a["feat"], I64(a["ffs"]), a["idx"], a["tr"],
        I64(a["cap"]), F32(a["bg"]), a["W"], a["H"], I64(a["Q"]), a["off"], a["pts"], a["cT"], a["cn"], a["g"], a["slot"],
        a["rec"], a["rs"], a["detach"], a["dfeat"], I64(a["dfs"]), a["goff"], a["scratch"], SZ(a["nbytes"]), None)


def _refused(lib, rc, word, fn):
    err = lib.splat_last_error()
    return rc == -1 and word in err and fn.encode() in err


def test_single_frame_entry_validates_before_hip(L):
    lib = L.lib()
    for bad in (dict(P=-1), dict(C=0), dict(W=0), dict(H=-2), dict(Q=-1), dict(cap=-1)):
        assert _refused(lib, _one(lib, **bad), b"sizes", ONE_), bad
    assert _refused(lib, _one(lib, W=(1 << 24) + 1), b"too large", ONE_)
    assert _refused(lib, _one(lib, Q=(1 << 29) + 1), b"too large", ONE_)
    for k in ("pts", "cT", "cn", "g", "uv", "conic", "op", "feat", "tr", "idx"):
        assert _refused(lib, _one(lib, **{k: None}), b"null", ONE_), k
    # the pair map: both halves, named in the message
    for k in ("goff", "slot"):
        assert _refused(lib, _one(lib, **{k: None}), b"pair map", ONE_), k
    assert _refused(lib, _one(lib, goff=None, slot=None), b"goff_incl", ONE_)
    # the scratch: missing, or one byte short of the documented size
    need = getattr(lib, ONE_ + "_scratch_bytes")(3, 64, 48, 5, 100)
    assert need == _documented(12, 5, 100 * 12)
    assert _refused(lib, _one(lib, scratch=None), b"scratch", ONE_)
    assert _refused(lib, _one(lib, nbytes=need - 1), b"scratch", ONE_)
    assert _refused(lib, _one(lib, nbytes=0), b"scratch", ONE_)


def test_batch_entry_validates_before_hip(L):
    lib = L.lib()
    for bad in (dict(F=0), dict(P=-1), dict(C=0), dict(W=0), dict(H=-2), dict(Q=-1), dict(cap=-1), dict(ofs=-1), dict(ffs=-1),
                dict(dfs=-1), dict(rs=4), dict(rs=18), dict(cap=0)):
        assert _refused(lib, _batch(lib, **bad), b"sizes", BATCH), bad
    assert _refused(lib, _batch(lib, H=(1 << 24) + 1), b"too large", BATCH)
    assert _refused(lib, _batch(lib, Q=(1 << 29) + 1), b"too large", BATCH)
    for k in ("pts", "off", "cT", "cn", "g", "uv", "conic", "op", "feat", "tr", "idx"):
        assert _refused(lib, _batch(lib, **{k: None}), b"null", BATCH), k
    for k in ("goff", "slot"):
        assert _refused(lib, _batch(lib, **{k: None}), b"pair map", BATCH), k
    need = getattr(lib, BATCH + "_scratch_bytes")(3, 3, 64, 48, 5, 100)
    assert need == _documented(36, 5, 3 * 100 * 4)
    assert _refused(lib, _batch(lib, scratch=None), b"scratch", BATCH)
    assert _refused(lib, _batch(lib, nbytes=need - 1), b"scratch", BATCH)


def test_nothing_to_do_is_valid_without_any_pointer(L):
    lib = L.lib()
    none = dict(uv=None, conic=None, op=None, feat=None, idx=None, tr=None, pts=None, cT=None, cn=None, g=None, goff=None, slot=None,
                scratch=None, nbytes=0)
    assert _one(lib, Q=0, duv=None, dconic=None, dop=None, dfeat=None, **none) == 0
    assert _batch(lib, Q=0, off=None, rec=None, dfeat=None, **none) == 0
    # no Gaussians / no output wanted: nothing to add to, as the atomic entries
    gauss = dict(uv=None, conic=None, op=None, feat=None, idx=None, tr=None, goff=None, slot=None, scratch=None, nbytes=0)
    assert _one(lib, P=0, **gauss) == 0
    assert _batch(lib, P=0, rec=None, **gauss) == 0
    assert _one(lib, duv=None, dconic=None, dop=None, dfeat=None, goff=None, slot=None, scratch=None, nbytes=0) == 0
    assert _batch(lib, rec=None, dfeat=None, goff=None, slot=None, scratch=None, nbytes=0) == 0


def test_the_deterministic_flag_does_not_refuse_the_ordered_entries(L):
    lib = L.lib()
    lib.splat_set_deterministic(1)
    try:
        # refused for the scratch, not for the flag: validation got past where the atomic entries refuse
        assert _refused(lib, _one(lib, nbytes=0), b"scratch", ONE_) and b"deterministic" not in lib.splat_last_error()
        assert _refused(lib, _batch(lib, nbytes=0), b"scratch", BATCH) and b"deterministic" not in lib.splat_last_error()
    finally:
        lib.splat_set_deterministic(0)


def test_python_layers_refuse_before_anything_runs(L):
    import torch
    import dptr.gs as gs
    from splatter_a_video_amd.frames import _parse_points
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    args = (z(4, 2), z(4, 3), z(4, 1), z(4, 3), z(0, dt=torch.int32), z(1, 2, dt=torch.int32), 0.0, 16, 16, z(2, 2))
    with pytest.raises(ValueError, match="differentiable"):
        gs.alpha_blending_points(*args, ordered=True)
    with pytest.raises(ValueError, match="pair map"):
        gs.alpha_blending_points(*args, differentiable=True, ordered=True)
    # "ordered" is a known key of the sparse set (the CPU feature is what is refused here, not the key)
    with pytest.raises(ValueError, match="feature"):
        _parse_points(dict(feature=z(4, 3), points=z(1, 2), offsets=z(3, dt=torch.int64), ordered=True), None, 2, 4)
    with pytest.raises(ValueError, match="unknown"):
        _parse_points(dict(feature=z(4, 3), order=True), None, 2, 4)
