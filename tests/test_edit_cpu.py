"""Appearance editing without a GPU: splat_blend_fit_color and splat_tile_loss_sum (csrc/edit.hip) exported, declared, listed and
refusing bad arguments with SPLAT_E_ARG before any HIP call; additions only, so the ABI version stays 22; select_gaussians on CPU
tensors against the reference's torch.unique formulation; and the argument validation of AppearanceFit / fit_appearance."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIT = "splat_blend_fit_color"
SUM = "splat_tile_loss_sum"
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
    for name in (FIT, SUM):
        assert name in L.SYMBOLS and hasattr(so, name) and name in declared, name
    lib = L.lib()
    assert len(lib.splat_blend_fit_color.argtypes) == 22
    assert len(lib.splat_tile_loss_sum.argtypes) == 5
    assert lib.splat_abi_version() == 22 and L.ABI_VERSION == 22
    assert re.search(r"#define SPLAT_ABI_VERSION 22\b", header)
    doc = header[header.index("splat_blend_fit_color, ONE launch"):][:3000]
    assert "No float atomics" in doc and "plain store" in doc
    import splatter_a_video_amd as pkg
    for name in ("AppearanceFit", "fit_appearance", "select_gaussians"):
        assert hasattr(pkg, name), name


def _fit(lib, **k):
    a = dict(P=10, C=3, uv=ONE, conic=ONE, op=ONE, feat=ONE, idx=ONE, tr=ONE, slot=ONE, cap=100, bg=0.0, W=64, H=48, target=ONE,
             pw=None, n=12, at=None, loss=ONE, grad=ONE, out=None, nc=None)
    a.update(k)
    return lib.splat_blend_fit_color(a["P"], a["C"], a["uv"], a["conic"], a["op"], a["feat"], a["idx"], a["tr"], a["slot"],
                                     I64(a["cap"]), F32(a["bg"]), a["W"], a["H"], a["target"], a["pw"], a["n"], a["at"], a["loss"],
                                     a["grad"], a["out"], a["nc"], None)


def test_fit_color_validates_before_hip(L):
    lib = L.lib()
    assert _fit(lib, P=0) == -1 and b"sizes" in lib.splat_last_error() and FIT.encode() in lib.splat_last_error()
    for bad in (dict(P=-3), dict(W=0), dict(H=-2), dict(cap=0), dict(cap=-1)):
        assert _fit(lib, **bad) == -1 and b"sizes" in lib.splat_last_error(), bad
    for C in (0, 1, 4, 32):
        assert _fit(lib, C=C) == -1 and b"C must be 3" in lib.splat_last_error(), C
    for k in ("uv", "conic", "op", "feat", "idx", "tr", "slot", "target", "loss", "grad"):
        assert _fit(lib, **{k: None}) == -1 and b"null" in lib.splat_last_error(), k
    for addr in (20, 24, 17):
        assert _fit(lib, grad=ctypes.c_void_p(addr)) == -1 and b"aligned" in lib.splat_last_error(), addr
    assert _fit(lib, n=-1) == -1 and b"n_active" in lib.splat_last_error()
    assert _fit(lib, n=-1, at=ONE) == -1 and b"n_active" in lib.splat_last_error()
    assert _fit(lib, n=13, at=ONE) == -1 and b"n_active" in lib.splat_last_error()      # 64 x 48: T = 12
    assert _fit(lib, n=5) == -1 and b"n_active must be T" in lib.splat_last_error()     # every tile: n_active = T
    assert _fit(lib, W=1 << 20, H=1 << 20, n=0) == -1 and b"too many" in lib.splat_last_error()
    # n_active == 0 is valid and launches nothing (no HIP call: this machine has no GPU)
    assert _fit(lib, n=0) == 0 and _fit(lib, n=0, at=ONE) == 0


def test_tile_loss_sum_validates_before_hip(L):
    lib = L.lib()
    call = lambda T=12, loss=ONE, hist=ONE, slot=0: lib.splat_tile_loss_sum(T, loss, hist, I64(slot), None)
    assert call(T=0) == -1 and b"sizes" in lib.splat_last_error() and SUM.encode() in lib.splat_last_error()
    assert call(T=-4) == -1 and call(slot=-1) == -1 and b"sizes" in lib.splat_last_error()
    assert call(loss=None) == -1 and b"null" in lib.splat_last_error()
    assert call(hist=None) == -1 and b"null" in lib.splat_last_error()


def _unique_formulation(gs_idx, mask, P):
    """src/trainer_fragGS.py:1014-1015"""
    g = gs_idx if gs_idx.dim() == 4 else gs_idx[None]
    sel = torch.unique(g[0][mask > 0])
    sel = sel[sel != -1]
    out = torch.zeros(P, dtype=torch.bool)
    out[sel.long()] = True
    return out


def test_select_gaussians_equals_the_unique_formulation():
    from splatter_a_video_amd.edit import select_gaussians
    gen = torch.Generator().manual_seed(5)
    H, W, K, P = 13, 17, 4, 60
    gs_idx = torch.randint(0, P, (H, W, K), generator=gen, dtype=torch.int32)
    gs_idx[torch.rand(H, W, K, generator=gen) < 0.4] = -1           # unused slots
    gs_idx[3, 4] = -1                                               # a masked pixel that lists nothing
    mask = torch.zeros(H, W)
    mask[2:9, 3:11] = 255.0
    mask[11, 0] = 0.5
    want = _unique_formulation(gs_idx, mask, P)
    assert 0 < int(want.sum()) < P
    for g in (gs_idx, gs_idx[None], gs_idx.long()):                 # a leading batch dimension, int64 ids
        got = select_gaussians(g, mask, P)
        assert got.dtype == torch.bool and got.shape == (P,) and torch.equal(got, want)
    assert torch.equal(select_gaussians(gs_idx, mask > 0, P), want)                     # a bool mask
    empty = select_gaussians(gs_idx, torch.zeros(H, W), P)                              # a mask of zeros
    assert empty.shape == (P,) and not empty.any()
    assert not select_gaussians(torch.full((H, W, K), -1, dtype=torch.int32), torch.ones(H, W), P).any()
    assert select_gaussians(gs_idx, mask, 0 + P).sum() == want.sum()
    with pytest.raises(ValueError, match=r"\[1, H, W, K\]"):
        select_gaussians(torch.stack([gs_idx, gs_idx]), mask, P)
    with pytest.raises(ValueError, match="mask must have shape"):
        select_gaussians(gs_idx, mask[:-1], P)
    with pytest.raises(ValueError, match="integer tensor"):
        select_gaussians(gs_idx.float(), mask, P)
    with pytest.raises(ValueError, match="names Gaussian"):
        select_gaussians(gs_idx, mask, 5)


def _geometry(P=6):
    return dict(uv=torch.zeros(P, 2), depth=torch.ones(P, 1), conic=torch.ones(P, 3), radius=torch.ones(P, dtype=torch.int32),
                tiles=torch.ones(P, dtype=torch.int32), opacity=torch.ones(P, 1), shs=torch.zeros(P, 16, 3), selected=None, W=32, H=16)


def test_appearance_fit_validation():
    from splatter_a_video_amd.edit import AppearanceFit, _check_run_options
    g = _geometry()
    for bad, match in ((dict(sh_rows="rest"), "sh_rows"), (dict(lr=0.0), "lr"), (dict(betas=(0.9, 1.0)), "betas"), (dict(eps=0.0), "eps"),
                       (dict(W=0), "W and H"), (dict(shs=torch.zeros(6, 4, 3)), r"\[P, 16, 3\]"), (dict(shs=torch.zeros(6, 48)), r"\[P, 16, 3\]"),
                       (dict(uv=torch.zeros(5, 2)), "agree with shs"), (dict(opacity=torch.ones(7, 1)), "agree with shs"),
                       (dict(selected=torch.ones(5, dtype=torch.bool)), "selected"), (dict(selected=torch.ones(6)), "selected"),
                       (dict(pixel_weight=torch.ones(32, 16)), "pixel_weight")):
        with pytest.raises(ValueError, match=match):
            AppearanceFit(**{**g, **bad})
    with pytest.raises(ValueError, match="CUDA"):          # well-formed arguments still need the GPU: no CPU path
        AppearanceFit(**g)
    assert _check_run_options(1000, 1e-4, 10) == (1000, 1e-4, 10)
    assert _check_run_options(3, float("-inf"), 1) == (3, float("-inf"), 1)
    for bad, match in (((0, 1e-4, 10), "max_iters"), ((2.5, 1e-4, 10), "max_iters"), ((10, float("nan"), 10), "tol"),
                       ((10, float("inf"), 10), "tol"), ((10, 1e-4, 0), "check_every"), ((10, 1e-4, -2), "check_every"),
                       ((10, 1e-4, 1.5), "check_every")):
        with pytest.raises(ValueError, match=match):
            _check_run_options(*bad)


def test_fit_appearance_validation():
    from splatter_a_video_amd.dynamics import FrameClock
    from splatter_a_video_amd.edit import fit_appearance
    N, W, H = 5, 32, 16
    clock = FrameClock(8)
    I = clock.interval_num
    model = {"position": torch.zeros(N, 3), "pos_cubic_node": torch.zeros(N, 4 * I * 3), "rotation": torch.ones(N, 4),
             "rot_poly_feat": torch.zeros(N, 4, 4), "rot_fourier_feat": torch.zeros(N, 8, 4), "opacity": torch.zeros(N, 1),
             "scaling": torch.zeros(N, 3), "shs": torch.zeros(N, 16, 3)}
    extr, target = torch.eye(4), torch.zeros(H, W, 3)
    call = lambda m=model, t=target, **k: fit_appearance(m, clock, 0, extr, W, H, t, **k)
    for bad, match in ((dict(tol=float("nan")), "tol"), (dict(check_every=0), "check_every"), (dict(max_iters=0), "max_iters"),
                       (dict(sh_rows="rest"), "sh_rows"), (dict(lr=-1.0), "lr"), (dict(iterations=5), "unknown fit options"),
                       (dict(num_idx=0), "num_idx"), (dict(mask=torch.ones(W, H)), "mask must have shape"),
                       (dict(t=torch.zeros(3, H, W)), "target must have shape")):
        with pytest.raises(ValueError, match=match):
            call(**bad)
    with pytest.raises(ValueError, match="lacks"):
        call(m={k: v for k, v in model.items() if k != "scaling"})
    with pytest.raises(ValueError, match="pass shs="):
        call(m={k: v for k, v in model.items() if k != "shs"})
    with pytest.raises(ValueError, match=r"\[N = 5, 16, 3\]"):
        call(shs=torch.zeros(N, 4, 3))
    with pytest.raises(TypeError, match="parameter dict or DynamicGaussians"):
        call(m=[1, 2])
    with pytest.raises(ValueError, match="CUDA"):          # well-formed arguments still need the GPU: no CPU path
        call()
