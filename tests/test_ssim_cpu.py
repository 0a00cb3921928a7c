"""SSIM entry points of the C ABI (csrc/loss.hip, ABI 22) without a GPU: exported, and every bad argument refused with SPLAT_E_ARG
before any HIP call; losses.ssim has no CPU fallback."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["splat_ssim_scratch_bytes", "splat_ssim_forward", "splat_ssim_backward", "splat_dssim_l1_loss_grad"]


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def _s(*v):
    return (ctypes.c_int64 * 4)(*v)


def test_ssim_symbols_are_exported(L):
    so = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(so, name), name
    assert L.lib().splat_abi_version() == L.ABI_VERSION == 22


def test_scratch_query(L):
    lib = L.lib()
    assert lib.splat_ssim_scratch_bytes(25, 3, 480, 854, 11) > 0
    assert lib.splat_ssim_scratch_bytes(25, 480, 854, 3, 11) > 0
    assert lib.splat_ssim_scratch_bytes(1, 1, 1, 1, 1) > 0 and lib.splat_ssim_scratch_bytes(1, 1, 1, 1, 15) > 0
    assert lib.splat_ssim_scratch_bytes(1, 3, 64, 64, 10) == 0          # even window
    assert lib.splat_ssim_scratch_bytes(1, 3, 64, 64, 17) == 0          # wider than 15
    assert lib.splat_ssim_scratch_bytes(-1, 3, 64, 64, 11) == 0


def test_ssim_entry_points_validate_before_hip(L):
    lib = L.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: every call below is refused on the host
    st = _s(3 * 64 * 64, 64 * 64, 64, 1)
    fwd = lambda N, C, H, W, win, a=one, b=one, sa=st, sb=st, mean=one, per=None, scr=one: lib.splat_ssim_forward(
        N, C, H, W, win, a, sa, b, sb, mean, per, scr, None)
    assert fwd(1, 3, 64, 64, 10) == -1 and b"odd" in lib.splat_last_error()
    assert fwd(1, 3, 64, 64, 0) == -1 and fwd(1, 3, 64, 64, 17) == -1
    assert fwd(-1, 3, 64, 64, 11) == -1 and b"sizes" in lib.splat_last_error()
    assert fwd(1, 3, -64, 64, 11) == -1 and fwd(1, 3, 64, 0, 11) == -1
    assert fwd(1, 3, 64, 64, 11, a=None) == -1 and b"null" in lib.splat_last_error()
    assert fwd(1, 3, 64, 64, 11, sb=None) == -1
    assert fwd(1, 3, 64, 64, 11, scr=None) == -1
    assert fwd(1, 3, 64, 64, 11, mean=None, per=None) == -1
    assert fwd(1, 3, 64, 64, 11, sa=_s(1, 1, -1, 1)) == -1 and b"strides" in lib.splat_last_error()
    bwd = lambda win, g=one, d=one, sd=st, N=1: lib.splat_ssim_backward(N, 3, 64, 64, win, one, st, one, st, g, 0, d, sd, 0, None)
    assert bwd(12) == -1 and bwd(11, N=-2) == -1
    assert bwd(11, g=None) == -1 and bwd(11, d=None) == -1 and bwd(11, sd=None) == -1
    f = ctypes.c_float
    dl = lambda win, grad=one, scr=one, N=1: lib.splat_dssim_l1_loss_grad(N, 3, 64, 64, win, one, st, one, st, f(0.8), f(0.2),
                                                                         grad, st, None, None, scr, None)
    assert dl(4) == -1 and dl(11, N=-1) == -1 and dl(11, grad=None) == -1 and dl(11, scr=None) == -1


def test_losses_refuse_cpu_tensors(L):
    import torch
    from splatter_a_video_amd import losses
    a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    with pytest.raises(ValueError):
        losses.ssim(a, b)
    with pytest.raises(ValueError):
        losses.dssim_l1(a, b)
    with pytest.raises(ValueError):
        losses.planes(a, "hwc")
