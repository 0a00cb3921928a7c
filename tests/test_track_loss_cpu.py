"""The 2-D track loss without a GPU: the C ABI entries (csrc/loss.hip) exported and every bad argument refused with SPLAT_E_ARG
before any HIP call; ``tracks.TrackTargets`` packing (truncation, raster sort with the file-order pairing, refusals);
``tracks.frame_weights``; and the float32 torch restatement of the trainer's term (src/trainer_fragGS.py:528-569, written here)
against the golden vectors of the reference's own functions (tests/golden/make_golden_track.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from splatter_a_video_amd.tracks import TrackTargets, frame_weights

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden", "track_loss.npz")
NEW = ["splat_track_loss_scratch_bytes", "splat_track_loss_grad"]


def restate(img, pixels, target, w, H, W, quantile=0.98):
    """one pair of the trainer's flow term in float32 torch (differentiable w.r.t. img [C, H, W]): the prediction at the sorted
    raster ``pixels`` [Q] paired with ``target`` [Q, 4] row by row, the confidence-weighted mean of the kept residuals
    (masked_l1_loss with its default normalize=True); returns (loss, n_visible, n_selected)"""
    X = ((img[0] + 1.0) * W) / 2.0
    Y = ((img[1] + 1.0) * H) / 2.0
    pix = torch.as_tensor(pixels, dtype=torch.int64)
    t = torch.as_tensor(target, dtype=torch.float32)
    conf = 1 - torch.sigmoid(t[:, 3])
    vis = (1 - torch.sigmoid(t[:, 2])) * conf > 0.5
    n = int(vis.sum())
    if n == 0:
        return img.sum() * 0.0, 0, 0
    px, py = X.reshape(-1)[pix][vis], Y.reshape(-1)[pix][vis]
    r = ((px - t[vis, 0]).abs() + (py - t[vis, 1]).abs()) / 2
    c = conf[vis] * torch.as_tensor(w, dtype=torch.float32)
    thr = torch.quantile(r.detach(), quantile)          # NaN when a residual is: then nothing is selected and the loss is 0
    sel = r <= thr
    return (r * c)[sel].sum() / (c[sel].sum() + 1e-8) / max(H, W), n, int(sel.sum())


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_track_symbols_are_exported_and_scratch_query(L):
    so = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(so, name), name
    lib = L.lib()
    assert lib.splat_abi_version() == 22
    assert lib.splat_track_loss_scratch_bytes(25, 25 * 25600) >= 25 * 25600 * 4 + 25 * 4
    assert lib.splat_track_loss_scratch_bytes(1, 0) > 0
    assert lib.splat_track_loss_scratch_bytes(0, 10) == 0 and lib.splat_track_loss_scratch_bytes(1, -1) == 0


def test_track_entry_point_validates_before_hip(L):
    lib = L.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: every call below is refused on the host
    st = (ctypes.c_int64 * 4)(3 * 48 * 64, 48 * 64, 64, 1)
    bad = (ctypes.c_int64 * 4)(3 * 48 * 64, -1, 64, 1)
    f = ctypes.c_float

    def call(F=2, H=48, W=64, C=3, track=one, ts=st, offs=one, pix=one, tgt=one, Q=10, fw=one, q=0.98, grad=None, gs=None,
             scr=one):
        return lib.splat_track_loss_grad(F, H, W, C, track, ts, offs, pix, tgt, Q, fw, f(q), f(1.0), grad, gs, 0,
                                         None, None, None, scr, None)
    assert call(F=0) == -1 and b"sizes" in lib.splat_last_error()
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=1) == -1 and call(Q=-1) == -1
    assert call(q=1.5) == -1 and b"quantile" in lib.splat_last_error()
    assert call(q=-0.1) == -1 and call(q=float("nan")) == -1
    assert call(track=None) == -1 and b"null" in lib.splat_last_error()
    assert call(ts=None) == -1 and call(offs=None) == -1 and call(fw=None) == -1 and call(scr=None) == -1
    assert call(pix=None) == -1 and call(tgt=None) == -1
    assert call(tgt=ctypes.c_void_p(20)) == -1 and b"aligned" in lib.splat_last_error()
    assert call(ts=bad) == -1 and b"strides" in lib.splat_last_error()
    assert call(grad=one, gs=None) == -1 and call(grad=one, gs=bad) == -1
    assert call(H=1 << 16, W=1 << 16) == -1


def test_track_targets_packing():
    H, W = 6, 8
    q = np.array([[3.9, 1.2], [-0.4, 0.0], [7.99, 5.5], [0.2, 2.7]], np.float32)
    t = np.arange(16, dtype=np.float32).reshape(4, 4)
    tt = TrackTargets.from_reference(q, t, H, W)
    # truncation toward zero: (3, 1), (0, 0), (7, 5), (0, 2) -> raster 11, 0, 47, 16, sorted; the rows stay in file order
    assert tt.pixels.tolist() == [0, 11, 16, 47]
    assert torch.equal(tt.targets, torch.from_numpy(t))
    assert tt.offsets.tolist() == [0, 4] and tt.counts == (4,) and (tt.F, tt.Q, tt.H, tt.W) == (1, 4, H, W)
    assert tt.pixels.dtype == torch.int32 and tt.offsets.dtype == torch.int64
    # [1, Q, 4] as load_target_tracks(ids1, [ids2], dim=0) returns it, torch inputs
    tt2 = TrackTargets.from_reference(torch.from_numpy(q), torch.from_numpy(t)[None], H, W)
    assert torch.equal(tt2.pixels, tt.pixels) and torch.equal(tt2.targets, tt.targets)
    b = TrackTargets.cat([tt, TrackTargets.from_reference(q[:2], t[:2], H, W), tt])
    assert b.offsets.tolist() == [0, 4, 6, 10] and b.counts == (4, 2, 4) and b.F == 3
    assert b.pixels.tolist() == [0, 11, 16, 47, 0, 11, 0, 11, 16, 47]
    assert TrackTargets.from_reference(np.zeros((0, 2)), np.zeros((0, 4)), H, W).Q == 0
    with pytest.raises(ValueError):
        TrackTargets.from_reference([[8.0, 0.0]], t[:1], H, W)          # x = W
    with pytest.raises(ValueError):
        TrackTargets.from_reference([[0.0, 6.2]], t[:1], H, W)          # y = H
    with pytest.raises(ValueError):
        TrackTargets.from_reference([[-1.0, 0.0]], t[:1], H, W)         # truncates to -1
    with pytest.raises(ValueError):
        TrackTargets.from_reference([[3.1, 1.0], [3.7, 1.9]], t[:2], H, W)    # both pixel (3, 1)
    with pytest.raises(ValueError):
        TrackTargets.from_reference(q, t[:3], H, W)
    with pytest.raises(ValueError):
        TrackTargets.from_reference([[float("nan"), 0.0]], t[:1], H, W)
    with pytest.raises(ValueError):
        TrackTargets.cat([tt, TrackTargets.from_reference(q, t, H + 1, W)])


def test_frame_weights_match_the_float32_formula():
    t1, t2, n = [0, 3, 7, 12, 5], [5, 1, 19, 2, 5], 20
    got = frame_weights(t1, t2, n)
    assert got.dtype == torch.float32
    want = torch.exp(-2 * torch.abs(torch.tensor(t2) - torch.tensor(t1)).float() / n)
    assert torch.equal(got, want)
    assert float(got[-1]) == 1.0


@pytest.mark.parametrize("case", ["grid", "shuffled", "ties", "nan"])
def test_restatement_reproduces_the_reference_fixture(case):
    g = np.load(GOLD)
    G = lambda k: g[f"{case}_{k}"]
    track = G("track")
    H, W = track.shape[-2:]
    tt = TrackTargets.from_reference(G("query_xy"), G("target"), H, W)
    w = frame_weights([int(G("ids1"))], [int(G("ids2"))], int(G("num_imgs")))[0]
    img = torch.from_numpy(track[0]).requires_grad_(True)
    loss, n, s = restate(img, tt.pixels, tt.targets, w, H, W)
    (grad,) = torch.autograd.grad(loss, [img])
    if case == "nan":          # a NaN residual: the quantile is NaN, nothing is kept, loss and gradient are 0
        assert n > 0 and s == 0 and float(loss.detach()) == 0.0 and float(G("loss")) == 0.0
    else:
        assert 0 < s <= n
    np.testing.assert_allclose(float(loss.detach()), float(G("loss")), rtol=1e-6)
    np.testing.assert_allclose(grad.numpy(), G("grad")[0], rtol=1e-5, atol=1e-7 * np.abs(G("grad")).max() + 1e-30)
    assert np.array_equal(grad.numpy() != 0, G("grad")[0] != 0)


def test_track_loss_refuses_cpu_tensors():
    from splatter_a_video_amd import losses
    tt = TrackTargets.from_reference([[1.0, 1.0]], [[1.0, 1.0, -5.0, -5.0]], 4, 4)
    with pytest.raises(ValueError):
        losses.track_loss(torch.zeros(1, 3, 4, 4), tt, torch.ones(1))
