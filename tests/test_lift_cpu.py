"""Feature lifting without a GPU: splat_blend_lift_batch, splat_lift_fold and splat_lift_pair_stride (csrc/lift.hip) exported,
declared, listed and refusing bad arguments with SPLAT_E_ARG before any HIP call; additions only, so the ABI version stays 22; and
the argument validation of blend_lift / FeatureLift / lift_features on CPU tensors."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIFT = "splat_blend_lift_batch"
FOLD = "splat_lift_fold"
STRIDE = "splat_lift_pair_stride"
ONE = ctypes.c_void_p(16)          # never dereferenced: every call of these tests is refused on the host
I64 = ctypes.c_int64


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_symbols_are_exported_declared_listed_and_the_abi_version_stays(L):
    so = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    declared = set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", header))
    for name in (LIFT, FOLD, STRIDE):
        assert name in L.SYMBOLS and hasattr(so, name) and name in declared, name
    lib = L.lib()
    assert len(lib.splat_blend_lift_batch.argtypes) == 20
    assert len(lib.splat_lift_fold.argtypes) == 12
    assert lib.splat_abi_version() == 22 and L.ABI_VERSION == 22
    assert re.search(r"#define SPLAT_ABI_VERSION 22\b", header)
    doc = header[header.index("feature lifting: per-Gaussian features"):][:4000]
    assert "No float atomics" in doc and "plain store" in doc and LIFT in doc and FOLD in doc
    import splatter_a_video_amd as pkg
    for name in ("FeatureLift", "blend_lift", "lift_features"):
        assert hasattr(pkg, name), name


def test_pair_stride(L):
    lib = L.lib()
    for cn in range(1, 33):
        for den in (0, 1):
            s = lib.splat_lift_pair_stride(cn, den)
            assert s % 4 == 0 and cn + den <= s < cn + den + 4, (cn, den, s)
    assert lib.splat_lift_pair_stride(0, 0) == 0 and lib.splat_lift_pair_stride(33, 1) == 0 and lib.splat_lift_pair_stride(-1, 1) == 0


def _lift(lib, **k):
    a = dict(F=2, P=10, D=40, c0=32, cn=8, uv=ONE, conic=ONE, op=ONE, ofs=10, idx=ONE, tr=ONE, slot=ONE, cap=100, W=64, H=48, maps=ONE,
             pw=None, den=1, rec=ONE)
    a.update(k)
    return lib.splat_blend_lift_batch(a["F"], a["P"], a["D"], a["c0"], a["cn"], a["uv"], a["conic"], a["op"], I64(a["ofs"]), a["idx"],
                                      a["tr"], a["slot"], I64(a["cap"]), a["W"], a["H"], a["maps"], a["pw"], a["den"], a["rec"], None)


def test_lift_batch_validates_before_hip(L):
    lib = L.lib()
    assert _lift(lib, P=0) == -1 and b"sizes" in lib.splat_last_error() and LIFT.encode() in lib.splat_last_error()
    for bad in (dict(F=0), dict(F=-1), dict(P=-3), dict(D=0), dict(W=0), dict(H=-2), dict(cap=0), dict(cap=-1), dict(ofs=-1)):
        assert _lift(lib, **bad) == -1 and b"sizes" in lib.splat_last_error(), bad
    for bad in (dict(cn=0), dict(cn=33, c0=0), dict(cn=-1), dict(c0=-1), dict(c0=33, cn=8), dict(D=39)):
        assert _lift(lib, **bad) == -1 and b"1..32 channels" in lib.splat_last_error(), bad
    for k in ("uv", "conic", "op", "idx", "tr", "slot", "maps", "rec"):
        assert _lift(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k
    for addr in (20, 24, 17):
        assert _lift(lib, rec=ctypes.c_void_p(addr)) == -1 and b"aligned" in lib.splat_last_error(), addr
    assert _lift(lib, W=1 << 20, H=1 << 20) == -1 and b"too many" in lib.splat_last_error()


def _fold(lib, **k):
    a = dict(F=2, P=10, cn=8, den_on=1, cap=100, goff=ONE, rec=ONE, num=ONE, stride=40, c0=32, den=ONE)
    a.update(k)
    return lib.splat_lift_fold(a["F"], a["P"], a["cn"], a["den_on"], I64(a["cap"]), a["goff"], a["rec"], a["num"], I64(a["stride"]),
                               a["c0"], a["den"], None)


def test_lift_fold_validates_before_hip(L):
    lib = L.lib()
    assert _fold(lib, P=0) == -1 and b"sizes" in lib.splat_last_error() and FOLD.encode() in lib.splat_last_error()
    for bad in (dict(F=0), dict(P=-3), dict(cap=0), dict(cap=-5)):
        assert _fold(lib, **bad) == -1 and b"sizes" in lib.splat_last_error(), bad
    for bad in (dict(cn=0), dict(cn=33, c0=0), dict(c0=-1), dict(stride=39), dict(c0=33)):
        assert _fold(lib, **bad) == -1 and b"1..32 channels" in lib.splat_last_error(), bad
    for k in ("goff", "rec", "num", "den"):
        assert _fold(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k
    for addr in (20, 24, 17):
        assert _fold(lib, rec=ctypes.c_void_p(addr)) == -1 and b"aligned" in lib.splat_last_error(), addr


def _model(N, clock):
    I = clock.interval_num
    return {"position": torch.zeros(N, 3), "pos_cubic_node": torch.zeros(N, 4 * I * 3), "rotation": torch.ones(N, 4),
            "rot_poly_feat": torch.zeros(N, 4, 4), "rot_fourier_feat": torch.zeros(N, 8, 4), "opacity": torch.zeros(N, 1),
            "scaling": torch.zeros(N, 3)}


def test_feature_lift_validation():
    from splatter_a_video_amd.dynamics import FrameClock
    from splatter_a_video_amd.lift import FeatureLift, lift_features
    N, W, H, D = 5, 32, 16, 3
    clock = FrameClock(8)
    model, extr = _model(N, clock), torch.eye(4)
    make = lambda m=model, **k: FeatureLift(m, clock, k.pop("extr", extr), k.pop("W", W), k.pop("H", H), k.pop("D", D), **k)
    for bad, match in ((dict(W=0), "W and H"), (dict(D=0), "D must be"), (dict(frames_per_batch=0), "frames_per_batch"),
                       (dict(frames_per_batch=2.5), "frames_per_batch"), (dict(capacity=0), "capacity"),
                       (dict(extr=torch.eye(3)), "extr"), (dict(cubic_layout=7), "cubic_layout")):
        with pytest.raises(ValueError, match=match):
            make(**bad)
    with pytest.raises(ValueError, match="lacks"):
        make(m={k: v for k, v in model.items() if k != "scaling"})
    with pytest.raises(ValueError, match="does not hold"):
        make(m={**model, "rotation": torch.ones(N + 1, 4)})
    with pytest.raises(TypeError, match="parameter dict or DynamicGaussians"):
        make(m=[1, 2])
    with pytest.raises(ValueError, match="CUDA"):          # well-formed arguments still need the GPU: no CPU path
        make()
    times, maps = [0, 1], torch.zeros(2, D, H, W)
    call = lambda mp=maps, pw=None, t=times, **k: lift_features(model, clock, t, extr, W, H, mp, pw, **k)
    for mp in (torch.zeros(D, H, W), torch.zeros(2, H, W, D), torch.zeros(3, D, H, W), torch.zeros(2, D, W, H), torch.zeros(2, 0, H, W)):
        with pytest.raises(ValueError, match=r"maps must have shape \[F, D, H, W\]"):
            call(mp=mp)
    with pytest.raises(ValueError, match="maps must be float32"):
        call(mp=maps.double())
    for pw in (torch.ones(H, W), torch.ones(2, W, H), torch.ones(2, 1, H, W), torch.ones(3, H, W)):
        with pytest.raises(ValueError, match=r"pixel_weight must have shape \[F, H, W\]"):
            call(pw=pw)
    with pytest.raises(ValueError, match="pixel_weight must be float32"):
        call(pw=torch.ones(2, H, W, dtype=torch.float64))
    with pytest.raises(TypeError, match="maps must be a torch.Tensor"):
        call(mp=[1.0])
    with pytest.raises(ValueError, match="CUDA"):
        call()
    with pytest.raises(ValueError, match="CUDA"):
        call(pw=torch.ones(2, H, W))


def test_blend_lift_validation():
    from splatter_a_video_amd.lift import blend_lift

    class PM:
        goff = torch.zeros(6, dtype=torch.int32)
        slot_sorted = torch.zeros(9, dtype=torch.int32)

    P, W, H, D = 6, 32, 16, 2
    g = dict(uv=torch.zeros(P, 2), conic=torch.ones(P, 3), opacity=torch.ones(P, 1), idx_sorted=torch.zeros(9, dtype=torch.int32),
             tile_range=torch.zeros(2, 2, dtype=torch.int32), pairmap=PM(), maps=torch.zeros(D, H, W), W=W, H=H)
    for bad, match in ((dict(W=0), "W and H"), (dict(uv=torch.zeros(5, 2)), "agree on P"), (dict(conic=torch.ones(P, 2)), "agree on P"),
                       (dict(tile_range=torch.zeros(3, 2, dtype=torch.int32)), "tile_range"),
                       (dict(maps=torch.zeros(D, W, H)), r"maps must have shape \[F, D, H, W\]"),
                       (dict(maps=torch.zeros(2, D, H, W)), r"maps must have shape \[F, D, H, W\]"),
                       (dict(maps=torch.zeros(D, H, W, dtype=torch.float16)), "maps must be float32"),
                       (dict(pixel_weight=torch.ones(W, H)), r"pixel_weight must have shape \[F, H, W\]"),
                       (dict(pairmap=None), "pair map")):
        with pytest.raises(ValueError, match=match):
            blend_lift(**{**g, **bad})
    with pytest.raises(ValueError, match="CUDA"):
        blend_lift(**g)
