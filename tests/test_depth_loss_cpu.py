"""The median-normalised depth loss without a GPU: the C ABI entries (csrc/loss.hip) exported and every bad argument refused
with SPLAT_E_ARG before any HIP call; the float32 torch restatement of the reference's ``depth_loss_dpt`` (tests/depth_ref.py)
against the golden vectors of the reference's own function (tests/golden/make_golden_depth.py); the closed-form gradient the
kernels implement against float64 autograd, tie split included; and, for every input of the GPU tests, that float32 itself stays
within the loss tolerance of float64."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import depth_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden", "depth_loss.npz")
NEW = ["splat_depth_dpt_scratch_bytes", "splat_depth_stats", "splat_depth_dpt_loss_grad"]
GOLD_CASES = ["smooth", "plateau", "odd", "signed", "nan"]


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_depth_symbols_are_exported_and_scratch_query(L):
    so = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(so, name), name
    lib = L.lib()
    assert lib.splat_abi_version() == 22
    q = lib.splat_depth_dpt_scratch_bytes
    sizes = [q(F, 480, 854) for F in (1, 2, 3, 25, 26, 100)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert q(25, 480, 854) >= 50 * 4 * 256 * 4          # four 256-bin histograms per image
    assert q(1, 1, 1) > 0
    assert q(0, 4, 4) == 0 and q(1, 0, 4) == 0 and q(1, 4, -1) == 0 and q(-1, 4, 4) == 0
    assert q(1, 1 << 16, 1 << 15) == 0 and q((1 << 24) + 1, 4, 4) == 0
    assert q(1, 1, (1 << 31) - 1) > 0


def test_chunk_constant_matches_the_source():
    from splatter_a_video_amd import losses
    src = open(os.path.join(ROOT, "splatter_a_video_amd", "csrc", "loss.hip")).read()
    threads = int(re.search(r"constexpr int DPT_THREADS = (\d+);", src).group(1))
    per = int(re.search(r"constexpr int DPT_PER = (\d+);", src).group(1))
    assert threads * per == losses.DEPTH_CHUNK == R.CH


def test_depth_entry_points_validate_before_hip(L):
    lib = L.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: every call below is refused on the host
    st = (ctypes.c_int64 * 4)(48 * 64, 48 * 64, 64, 1)
    bad = (ctypes.c_int64 * 4)(48 * 64, 48 * 64, -1, 1)
    f = ctypes.c_float

    def call(F=2, H=48, W=64, pred=one, ps=st, gt=one, gs=st, gstats=None, grad=None, grs=None, scr=one):
        return lib.splat_depth_dpt_loss_grad(F, H, W, pred, ps, gt, gs, gstats, f(1.0), grad, grs, 0, None, None, None, None, scr,
                                             None)
    assert call(F=0) == -1 and b"sizes" in lib.splat_last_error()
    assert call(H=0) == -1 and call(W=-3) == -1 and call(F=-1) == -1
    assert call(H=1 << 16, W=1 << 15) == -1 and b"too large" in lib.splat_last_error()
    assert call(F=(1 << 24) + 1) == -1 and b"too large" in lib.splat_last_error()
    assert call(pred=None) == -1 and b"null" in lib.splat_last_error()
    assert call(ps=None) == -1 and call(gt=None) == -1 and call(gs=None) == -1 and call(scr=None) == -1
    assert call(ps=bad) == -1 and b"strides" in lib.splat_last_error()
    assert call(gs=bad) == -1
    assert call(grad=one, grs=None) == -1 and b"null" in lib.splat_last_error()
    assert call(grad=one, grs=bad) == -1 and b"strides" in lib.splat_last_error()

    def stats(F=2, H=48, W=64, img=one, s=st, out=one, scr=one):
        return lib.splat_depth_stats(F, H, W, img, s, out, scr, None)
    assert stats(F=0) == -1 and stats(H=0) == -1 and stats(W=0) == -1 and b"sizes" in lib.splat_last_error()
    assert stats(H=1 << 16, W=1 << 15) == -1 and stats(F=(1 << 24) + 1) == -1
    assert stats(img=None) == -1 and stats(s=None) == -1 and stats(out=None) == -1 and stats(scr=None) == -1
    assert b"null" in lib.splat_last_error()
    assert stats(s=bad) == -1 and b"strides" in lib.splat_last_error()


def test_depth_wrappers_refuse_cpu_tensors_and_weight():
    from splatter_a_video_amd import losses
    z = torch.zeros(4, 4, 1)
    with pytest.raises(ValueError):
        losses.depth_loss_dpt(z, z)
    with pytest.raises(NotImplementedError):
        losses.depth_loss_dpt(z, z, weight=z)
    with pytest.raises(ValueError):
        losses.depth_stats(torch.zeros(1, 1, 4, 4))
    with pytest.raises(ValueError):
        losses.depth_dpt_loss_grad(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_loss_weights_has_the_off_switch():
    from splatter_a_video_amd.train_step import LossWeights
    assert LossWeights().depth_dpt == 0.0 and LossWeights().depth == 1.0


@pytest.mark.parametrize("case", GOLD_CASES)
def test_restatement_reproduces_the_reference_fixture(case):
    g = np.load(GOLD)
    pred, gt = g[f"{case}_pred"], g[f"{case}_gt"]
    assert pred.shape == ((39, 55) if case == "odd" else (40, 56))
    p = torch.from_numpy(pred)[..., None].clone().requires_grad_(True)
    loss = R.restate(p, torch.from_numpy(gt)[..., None])
    (grad,) = torch.autograd.grad(loss, [p])
    grad = grad[..., 0].numpy()
    if case == "nan":
        assert np.isnan(float(loss.detach())) and np.isnan(g["nan_loss"])
        assert np.isnan(grad).all() and np.isnan(g["nan_grad"]).all()
        return
    np.testing.assert_allclose(float(loss.detach()), float(g[f"{case}_loss"]), rtol=1e-6)
    R.assert_grad_tol(grad, g[f"{case}_grad"], case)
    if case == "plateau":          # the median is inside the plateau
        assert R.lower_median(pred) == 1.0 and (pred == 1.0).sum() > pred.size // 2
    if case == "signed":
        assert (gt < 0).any() and (gt > 0).any() and (gt == 0).sum() >= 12 and np.signbit(gt[gt == 0]).any()


def _tie_case():
    """m = 3 pixels at the median, S = 3 != 0"""
    p = np.array([1, 3, 2, 2, 5, 2, 7, 8], np.float32)
    g = np.array([0.3, -1.0, 2.5, 0.1, 0.7, -0.2, 1.9, 0.4], np.float32)
    assert R.lower_median(p) == 2 and (p == 2).sum() == 3 and np.sign(p - 2).sum() == 3
    return p, g


@pytest.mark.parametrize("case", GOLD_CASES[:-1] + ["ties"])
def test_closed_form_gradient_is_float64_autograd(case):
    if case == "ties":
        pred, gt = _tie_case()
    else:
        g = np.load(GOLD)
        pred, gt = g[f"{case}_pred"], g[f"{case}_gt"]
    loss, grad = R.closed_form(pred, gt)
    want_loss, want, _, m = R.restate64(pred, gt)
    if case in ("plateau", "ties"):
        assert m > 1
    np.testing.assert_allclose(loss, want_loss, rtol=1e-12)
    np.testing.assert_allclose(grad.reshape(pred.shape), want, rtol=1e-9, atol=1e-12 * np.abs(want).max())


def test_median_gradient_is_split_evenly_over_the_ties():
    x = torch.tensor([1.0, 3.0, 2.0, 2.0, 5.0, 2.0], dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(torch.median(x), [x])
    assert torch.equal(g, torch.tensor([0, 0, 1, 1, 0, 1], dtype=torch.float64) / 3)


@pytest.mark.parametrize("case", R.LOSS_CASES)
def test_float32_stays_within_the_loss_tolerance_on_the_gpu_inputs(case):
    """the GPU tests compare s, the per-frame loss and the slot at rtol 1e-5: on each of their inputs the float32 torch
    restatement is already that close to float64 (|d| is of order 1: no difference of nearly equal numbers)"""
    pred, gt = R.inputs(case)
    for f in range(pred.shape[0]):
        want, _, st, _ = R.restate64(pred[f], gt[f])
        p, g = torch.from_numpy(pred[f]).reshape(-1), torch.from_numpy(gt[f]).reshape(-1)
        np.testing.assert_allclose(float(R.restate(p, g)), want, rtol=1e-5)
        np.testing.assert_allclose(float((p - torch.median(p)).abs().mean()), st[1], rtol=1e-5)
        assert np.isfinite(want) and want > 0.05
