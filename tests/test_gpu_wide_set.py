"""The WIDE detached set of the frame batch (``FrameBatch.render_sets`` / ``render_dynamic_sets(wide=...)``): a feature set of any
width composited beside the row over the batch's sorted lists in chunks of 32 channels (reference: render_attributes blended
with opacity.detach(), dptr_ortho_enhanced.py:361-376; alpha_blending.cu:287-394, 440-577).  Kernels under test: blend_fwd /
the tile backward kernels of every chunk width on a channel window of a frame batch (splat_alpha_blending_forward_batch_set,
splat_alpha_blending_backward_batch_set_packed),
frames_wide_fold_kernel (splat_frames_wide_fold) and the unchanged Gaussian-side walks behind it.

(1, 2) against the CPU oracle chain, the wide set being one more ``detach_opacity`` set of it; (3) the row is untouched; (4) the
same 16 attributes as ``wide=`` and inside the row; (5) stale records; (6) deterministic mode; (7) a training run with 40
attributes; (8) the step's loss terms keep their definitions.  Tolerances and caps are those of the neighbouring tests (test_gpu_frames_oracle.py, test_gpu_points_batch.py)."""
import os

import numpy as np
import pytest
import torch

import oracle_chain as oc
from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import train_step as TS
from splatter_a_video_amd.dynamics import SEGMENT_MAJOR, FrameClock, to_gaussian_major, to_segment_major
from splatter_a_video_amd.frames import FrameBatch
from splatter_a_video_amd.gs.raster_ops import capture_T_front
from splatter_a_video_amd.synth import make_scene
from test_gpu_parity import GRAD_RTOL, IMG_ATOL, IMG_RTOL, assert_grad
from test_gpu_train_step import _perturbed

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DYN = ("position", "pos_cubic_node", "rotation", "rot_poly_feat", "rot_fourier_feat", "opacity", "scaling")


def _t(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda", requires_grad=grad)


def _share_off(got, want):
    a = got.detach().cpu().numpy()
    return float((np.abs(a - want) > (IMG_ATOL + IMG_RTOL * np.abs(want))).mean())


# --------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("view", [(96, 64), (100, 70)], ids=["96x64", "100x70"])
@pytest.mark.parametrize("c", [1, 21, 32, 33, 64, 70])
def test_dynamic_route_against_oracle(oracle_mod, c, view):
    """the set-up of test_render_dynamic_sets_against_oracle_with_reference_parameters (reference-made dynamic fixture, 6 frames,
    K = 8) with rgb (taps) | depth | a 3-channel per-frame list in the row and a wide set of c channels beside it: one narrow
    chunk (1), the width no plan holds (21), a full chunk (32), a full chunk + 1 (33), two full chunks (64), two + a tail (70);
    96 x 64 and 100 x 70 (partial edge tiles).  Images and ids under the geometry-bound caps, every gradient under GRAD_RTOL (5e-3
    when a radius flipped on a rounding tie), as the neighbouring oracle tests."""
    W, H = view
    g = dict(np.load(os.path.join(GOLD, "dynamic_400x50.npz")))
    clock = FrameClock(int(g["T"]), g["intervals"], int(g["start_frame_id"]), int(g["time_len"]))
    I = clock.interval_num
    host = {k: np.ascontiguousarray(g[k], np.float32) for k in DYN}
    N, K = host["position"].shape[0], 8
    times = [int(t) for t in g["times"]][:6]
    F = len(times)
    extr = np.eye(4, dtype=np.float32)
    extr[0, 0] = extr[1, 1] = 0.3; extr[2, 2] = 0.1; extr[2, 3] = 2.0
    host["scaling"] = host["scaling"] + 2.0
    rng = np.random.default_rng(8)
    rgb = rng.uniform(size=(N, 3)).astype(np.float32)
    trk = rng.uniform(-1, 1, size=(F, N, 3)).astype(np.float32)          # per frame, as track_gs = position(ids2)
    wide = rng.uniform(-1, 1, size=(N, c)).astype(np.float32)
    gs_ = [rng.normal(size=(F, n, H, W)).astype(np.float32) for n in (3, 1, 3, c)]
    p = {k: _t(v, k not in ("rot_poly_feat", "rot_fourier_feat", "position")) for k, v in host.items()}
    p["pos_cubic_node"] = to_segment_major(_t(host["pos_cubic_node"]), I).requires_grad_(True)
    t_rgb, t_trk, t_wide = _t(rgb, True), _t(trk, True), _t(wide, True)
    B = FrameBatch(F, N, W, H, 7, "cuda", want_abs=True)
    sets = [dict(feature=t_rgb, bg=0.2, taps=True), dict(feature="depth", bg=1.0), dict(feature=[t_trk], bg=0.0, detach_opacity=True)]
    o_rgb, o_dep, o_trk, o_wide, ids = B.render_dynamic_sets(
        clock, times, _t(extr), sets, position=p["position"], pos_cubic_node=p["pos_cubic_node"], rotation=p["rotation"],
        rot_poly_feat=p["rot_poly_feat"], rot_fourier_feat=p["rot_fourier_feat"], opacity=p["opacity"], scaling=p["scaling"],
        cubic_layout=SEGMENT_MAJOR, K=K, wide=dict(feature=t_wide, bg=0.1, detach_opacity=True))
    assert tuple(o_wide.shape) == (F, c, H, W) and o_wide.requires_grad
    with capture_T_front() as cap:
        torch.autograd.backward([o_rgb, o_dep, o_trk, o_wide], [_t(x) for x in gs_])
    torch.cuda.synchronize()
    B.check()
    assert len(cap.maps) == 1 + (c + 31) // 32           # the row's replay, then one per chunk: each reproduced its forward
    for m in cap.maps:
        assert float((m - 1).abs().max()) < 2e-4
    # ---- the oracle, frame by frame (the row's third set differs from frame to frame)
    per, tot, d_trk = [], None, []
    for f, t in enumerate(times):
        osets = [dict(feature=rgb, bg=0.2, taps=True), dict(feature="depth", bg=1.0), dict(feature=trk[f], bg=0.0, detach_opacity=True),
                 dict(feature=wide, bg=0.1, detach_opacity=True)]
        pf, tf = oc.dynamic_frames(oracle_mod, clock, [t], host, extr, W, H, osets, [x[f:f + 1] for x in gs_], K=K)
        per += pf
        d_trk.append(tf["feats"][2])
        if tot is None:
            tot = dict(tf)
        else:
            for k in ("position", "pos_cubic_node", "rotation", "opacity", "scaling", "tap", "abs_tap"):
                tot[k] = tot[k] + tf[k]
            tot["feats"] = [None if a is None else a + b for a, b in zip(tot["feats"], tf["feats"])]
    assert sum(r["M"] for r in per) > 2000      # the view is populated
    rad = B.radius.cpu().numpy()
    same = all((rad[f] == r["radius"]).all() for f, r in enumerate(per))
    got = torch.cat([o_rgb, o_dep, o_trk, o_wide], 1)
    for f, r in enumerate(per):
        assert (rad[f] != r["radius"]).mean() <= 1e-4
        c0 = 0
        for img in r["imgs"]:
            assert _share_off(got[f, c0:c0 + img.shape[0]], img) < 1e-3, (f, c0)
            c0 += img.shape[0]
        assert (ids[f].cpu().numpy() != r["gs_idx"]).any(-1).mean() < 2e-3
    tol = GRAD_RTOL if same else 5e-3
    assert_grad(to_gaussian_major(p["pos_cubic_node"].grad).reshape(N, 4, I, 3), tot["pos_cubic_node"], "pos_cubic_node", tol)
    for k in ("rotation", "opacity", "scaling"):
        assert_grad(p[k].grad, tot[k], k, tol)
    assert_grad(t_rgb.grad, tot["feats"][0], "rgb", tol)
    assert_grad(t_trk.grad, np.stack(d_trk), "row attributes (per frame)", tol)
    assert_grad(t_wide.grad, tot["feats"][3], "wide feature", tol)
    assert_grad(B.tap, tot["tap"], "tap", tol)
    assert_grad(B.abs_tap, tot["abs_tap"], "abs_tap", tol)


# --------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("c", [33, 64])
def test_static_route_against_oracle(oracle_mod, c):
    """the same through render_sets on the reference-made orthographic fixture (1k Gaussians, 64 x 48), F = 3, against
    oc.static_frames"""
    g = dict(np.load(os.path.join(GOLD, "ortho_1k_64x48.npz")))
    F, K = 3, 8
    N, W, H = g["xyz"].shape[0], int(g["W"]), int(g["H"])
    rng = np.random.default_rng(21)
    opacity = (1.0 / (1.0 + np.exp(-rng.normal(0.0, 1.5, size=(N, 1))))).astype(np.float32)
    off = np.zeros((F, N, 3), np.float32)
    for f in range(1, F):
        d = 0.05 * np.sin(2.0 * np.pi * f / 7.0 + rng.uniform(0, 2 * np.pi, size=N))
        off[f, :, 0] = d; off[f, :, 1] = -0.5 * d
    rgb = rng.uniform(size=(N, 3)).astype(np.float32)
    att = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    wide = rng.uniform(-1, 1, size=(N, c)).astype(np.float32)
    gs_ = [rng.normal(size=(F, n, H, W)).astype(np.float32) for n in (3, 1, 3, c)]
    p = {k: _t(v, True) for k, v in dict(xyz=g["xyz"], scales=g["scale"], uquats=g["rotate"], opacity=opacity, rgb=rgb, att=att,
                                         wide=wide).items()}
    B = FrameBatch(F, N, W, H, 7, "cuda", want_abs=True)
    sets = [dict(feature=p["rgb"], bg=0.2, taps=True), dict(feature="depth", bg=1.0), dict(feature=p["att"], bg=0.0, detach_opacity=True)]
    o_rgb, o_dep, o_att, o_wide, ids = B.render_sets(p["xyz"], p["scales"], p["uquats"], p["opacity"], sets, _t(off), _t(g["extr"]), K=K,
                                                     wide=dict(feature=p["wide"], detach_opacity=True))
    assert tuple(o_wide.shape) == (F, c, H, W)
    with capture_T_front() as cap:
        torch.autograd.backward([o_rgb, o_dep, o_att, o_wide], [_t(x) for x in gs_])
    torch.cuda.synchronize()
    B.check()
    for m in cap.maps:
        assert float((m - 1).abs().max()) < 2e-4
    osets = [dict(feature=rgb, bg=0.2, taps=True), dict(feature="depth", bg=1.0), dict(feature=att, bg=0.0, detach_opacity=True),
             dict(feature=wide, bg=0.0, detach_opacity=True)]
    per, tot = oc.static_frames(oracle_mod, g["xyz"], off, g["scale"], g["rotate"], opacity, g["extr"], W, H, osets, gs_, K=K)
    rad = B.radius.cpu().numpy()
    same = all((rad[f] == r["radius"]).all() for f, r in enumerate(per))
    got = torch.cat([o_rgb, o_dep, o_att, o_wide], 1)
    for f, r in enumerate(per):
        assert (rad[f] != r["radius"]).mean() <= 1e-4
        c0 = 0
        for img in r["imgs"]:
            assert _share_off(got[f, c0:c0 + img.shape[0]], img) < 1e-3, (f, c0)
            c0 += img.shape[0]
        assert (ids[f].cpu().numpy() != r["gs_idx"]).any(-1).mean() < 2e-3
    tol = GRAD_RTOL if same else 5e-3
    assert_grad(p["xyz"].grad, tot["xyz"], "xyz", tol)
    assert_grad(p["scales"].grad, tot["scale"], "scales", tol)
    assert_grad(p["uquats"].grad, tot["rotate"], "uquats", tol)
    assert_grad(p["opacity"].grad, tot["opacity"], "opacity", tol)
    assert_grad(p["rgb"].grad, tot["feats"][0], "rgb", tol)
    assert_grad(p["att"].grad, tot["feats"][2], "row attributes", tol)
    assert_grad(p["wide"].grad, tot["feats"][3], "wide feature", tol)
    assert_grad(B.tap, tot["tap"], "tap", tol)
    assert_grad(B.abs_tap, tot["abs_tap"], "abs_tap", tol)


# --------------------------------------------------------------------------------------------------------------------- clip
NAMES = ("pos_cubic_node", "rotation", "opacity", "scaling")


def _clip(N=2500, W=128, H=96, T=20, seed=11, A=16, bigger=0.0):
    """a make_scene clip as the training-step tests build it: dynamic parameters, SH-free rgb, A attributes"""
    sc = make_scene(N, W, H, F=T, seed=seed, sigma_px=3.0)
    clock = FrameClock(T)
    truth = TS.synthetic_video_params(sc, clock, "cuda", attrs=A, seed=seed + 1, cubic_sigma=0.01)
    truth["pos_cubic_node"] = to_segment_major(truth["pos_cubic_node"], clock.interval_num)
    truth["scaling"] = truth["scaling"] + bigger
    rng = np.random.default_rng(seed + 2)
    return dict(clock=clock, extr=_t(sc.extr), par=truth, rgb=rng.uniform(size=(N, 3)).astype(np.float32), N=N, W=W, H=H)


def _leaves(cl):
    lv = {k: cl["par"][k].detach().clone().requires_grad_(True) for k in NAMES}
    lv["rgb"] = _t(cl["rgb"], True)
    lv["attrs"] = cl["par"]["attrs"].detach().clone().requires_grad_(True)
    return lv


def _render(fb, cl, lv, times, sets, **kw):
    par = cl["par"]
    return fb.render_dynamic_sets(cl["clock"], times, cl["extr"], sets, position=par["position"], pos_cubic_node=lv["pos_cubic_node"],
                                  rotation=lv["rotation"], rot_poly_feat=par["rot_poly_feat"], rot_fourier_feat=par["rot_fourier_feat"],
                                  opacity=lv["opacity"], scaling=lv["scaling"], cubic_layout=SEGMENT_MAJOR, **kw)


def _grads(lv, fb):
    out = {k: v.grad.detach().clone() for k, v in lv.items() if v.grad is not None}
    out["tap"] = fb.tap.clone()
    return out


TIMES = [0, 7, 13]


def _wide_call(fb, cl, lv, gimgs, grad_wide=True, sink=None, K=8):
    """rgb (taps) | depth in the row, the attributes beside it; backward with (or without) a gradient for the wide image"""
    sets = [dict(feature=lv["rgb"], bg=0.1, taps=True), dict(feature="depth", bg=1.0)]
    out = _render(fb, cl, lv, TIMES, sets, K=K, wide=dict(feature=lv["attrs"], bg=0.0, detach_opacity=True), grad_sink=sink)
    torch.autograd.backward(list(out[:3]) if grad_wide else list(out[:2]), gimgs[:3] if grad_wide else gimgs[:2])
    return out


def _gimgs(cl, A, seed=5):
    rng = np.random.default_rng(seed)
    return [_t(rng.normal(size=(len(TIMES), n, cl["H"], cl["W"]))) for n in (3, 1, A)]


# --------------------------------------------------------------------------------------------------------------------- 3
def test_the_row_is_untouched():
    """with wide= the row's images and ids are those of a call without it, bit for bit; with no gradient for the wide image
    (nothing of the wide set is launched in the backward) every gradient is, too"""
    cl = _clip()
    gim = _gimgs(cl, 16)
    F, N, W, H = len(TIMES), cl["N"], cl["W"], cl["H"]
    a, b = _leaves(cl), _leaves(cl)
    fa, fbb = FrameBatch(F, N, W, H, 4, "cuda"), FrameBatch(F, N, W, H, 4, "cuda")
    sets = [dict(feature=a["rgb"], bg=0.1, taps=True), dict(feature="depth", bg=1.0)]
    oa = _render(fa, cl, a, TIMES, sets, K=8)
    torch.autograd.backward(list(oa[:2]), gim[:2])
    ob = _wide_call(fbb, cl, b, gim, grad_wide=False)
    torch.cuda.synchronize()
    assert len(oa) == 3 and len(ob) == 4 and tuple(ob[2].shape) == (F, 16, H, W)
    assert torch.equal(oa[0], ob[0]) and torch.equal(oa[1], ob[1]) and torch.equal(oa[-1], ob[-1])
    ga, gb = _grads(a, fa), _grads(b, fbb)
    assert "attrs" not in gb and set(ga) == set(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    assert float(ob[2].detach().abs().max()) > 0


# --------------------------------------------------------------------------------------------------------------------- 4
def test_same_result_as_the_row_route():
    """16 attributes as wide= against the same 16 inside the row (the one-pass plan 3 | 1 | 16: today's path) on a 2 500-Gaussian
    clip at 128 x 96, F = 3.  Two float32 routes of one quantity, each under the project's gradient criterion 2e-3 |ref| + 1e-4
    max |ref| against the exact value: compared under twice that bound, element by element (tests/test_gpu_points_batch.py).
    Images: IMG_ATOL + IMG_RTOL |ref| on all but the 1e-3 share of pixels every image comparison here allows."""
    cl = _clip()
    gim = _gimgs(cl, 16)
    F, N, W, H = len(TIMES), cl["N"], cl["W"], cl["H"]
    a, b = _leaves(cl), _leaves(cl)
    fa, fbb = FrameBatch(F, N, W, H, 20, "cuda"), FrameBatch(F, N, W, H, 4, "cuda")
    sets = [dict(feature=a["rgb"], bg=0.1, taps=True), dict(feature="depth", bg=1.0), dict(feature=a["attrs"], bg=0.0, detach_opacity=True)]
    oa = _render(fa, cl, a, TIMES, sets, K=8)
    torch.autograd.backward(list(oa[:3]), gim)
    ob = _wide_call(fbb, cl, b, gim)
    torch.cuda.synchronize()
    for x, y in zip(oa[:3], ob[:3]):
        assert _share_off(y, x.detach().cpu().numpy()) < 1e-3
    assert torch.equal(oa[-1], ob[-1])
    ref, got = _grads(a, fa), _grads(b, fbb)
    assert set(ref) == set(got) and "attrs" in got
    for k in ref:
        r, x = ref[k].double().cpu().numpy().reshape(-1), got[k].double().cpu().numpy().reshape(-1)
        assert np.isfinite(x).all() and np.abs(r).max() > 0, k
        lim = 2.0 * (2e-3 * np.abs(r) + 1e-4 * np.abs(r).max())
        err = np.abs(x - r)
        print(f"wide vs row: d{k} max |ref| {np.abs(r).max():.3e}, worst err / bound {float((err / lim).max()):.4f}")
        assert (err <= lim).all(), f"d{k}: {int((err > lim).sum())} of {x.size} off, worst {float((err / lim).max()):.2f} x the bound"


# --------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "default"])
def test_stale_records(det):
    """a larger scene (every Gaussian twice as wide: more pairs, every record buffer filled further), then the clip itself on the
    SAME batch: the second call's gradients are those of a fresh batch -- nothing a chunk's tail records or the row's records
    held before is read.  Bit for bit in deterministic mode.  In the default mode the tile kernel of a chunk adds the survivors it
    carried over a super-batch boundary with float atomics, in arrival order (blend_bwd_mfma_kernel): its bits are not defined run
    to run, and the two batches are compared under the two-route bound of test 4 -- stale records would be O(1) off."""
    big, cl = _clip(bigger=0.7), _clip()
    A = 40
    for x in (big, cl):
        x["par"]["attrs"] = _t(np.random.default_rng(3).uniform(-1, 1, size=(x["N"], A)))
    gim = _gimgs(cl, A)
    F, N, W, H = len(TIMES), cl["N"], cl["W"], cl["H"]
    L.set_deterministic(det)
    try:
        used = FrameBatch(F, N, W, H, 4, "cuda")
        _wide_call(used, big, _leaves(big), gim)
        m_big = used.check()
        b = _leaves(cl)
        _wide_call(used, cl, b, gim)
        assert used.check() < 0.8 * m_big
        fresh = FrameBatch(F, N, W, H, 4, "cuda")
        a = _leaves(cl)
        _wide_call(fresh, cl, a, gim)
        torch.cuda.synchronize()
    finally:
        L.set_deterministic(False)
    ref, got = _grads(a, fresh), _grads(b, used)
    assert set(ref) == set(got) and "attrs" in got
    for k in ref:
        if det:
            assert torch.equal(ref[k], got[k]), k
        else:
            r, x = ref[k].double().cpu().numpy().reshape(-1), got[k].double().cpu().numpy().reshape(-1)
            assert (np.abs(x - r) <= 2.0 * (2e-3 * np.abs(r) + 1e-4 * np.abs(r).max())).all(), k


# --------------------------------------------------------------------------------------------------------------------- 6
def test_deterministic_mode():
    """the call runs under splat_set_deterministic(1) (no kernel with float atomics is launched) and two runs give bit-equal
    gradients, grad_sink["wide"] included"""
    cl = _clip()
    A = 40
    cl["par"]["attrs"] = _t(np.random.default_rng(3).uniform(-1, 1, size=(cl["N"], A)))
    gim = _gimgs(cl, A)
    F, N, W, H = len(TIMES), cl["N"], cl["W"], cl["H"]
    L.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            fb = FrameBatch(F, N, W, H, 4, "cuda")
            lv = _leaves(cl)
            sink = {"wide": torch.zeros(N, A, device="cuda")}
            _wide_call(fb, cl, lv, gim, sink=sink)
            torch.cuda.synchronize()
            assert lv["attrs"].grad is None and float(sink["wide"].abs().max()) > 0
            g = _grads(lv, fb)
            g["wide"] = sink["wide"]
            runs.append(g)
    finally:
        L.set_deterministic(False)
    assert set(runs[0]) == set(runs[1])
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


# --------------------------------------------------------------------------------------------------------------------- 7
def test_training_step_with_forty_attributes():
    """TrainingStep with attrs [N, 40]: the row is rgb | depth | track_gs, the 40 attributes form the wide set.  Set-up and
    assertions of test_training_step_with_the_trainers_small_attribute_rows; render_ground_truth returns the same dict."""
    A = 40
    Nn, Ww, Hh, T, F = 2500, 128, 96, 20, 3
    sc = make_scene(Nn, Ww, Hh, F=T, seed=11, sigma_px=3.0)
    clock = FrameClock(T)
    truth = TS.synthetic_video_params(sc, clock, "cuda", attrs=A, seed=12, cubic_sigma=0.01)
    extr = _t(sc.extr)
    lr = dict(TS.REFERENCE_LR, pos_cubic_node=2e-3, shs=2e-2, attrs=2e-2, scaling=1e-2, rotation=5e-3)
    st = TS.TrainingStep(_perturbed(truth, 1), clock, Ww, Hh, F, extr, lr=lr, K=8, arap_samples=128, sample_seed=3)
    assert st.wide and st.fb.C == 7
    t1, t2 = [0, 7, 13], [4, 2, 19]
    gt = TS.render_ground_truth(truth, clock, Ww, Hh, extr, t1, t2)
    assert gt["attr"].shape == (F, 3 + A, Hh, Ww) and gt["rgb"].shape == (F, 3, Hh, Ww) and gt["depth"].shape == (F, 1, Hh, Ww)
    before = {k: v.detach().clone() for k, v in st.p.items()}
    losses = []
    for _ in range(12):
        st.step(t1, t2, gt)
        losses.append(st.loss())
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    for k in TS.TRAINABLE:
        assert torch.isfinite(st.p[k]).all() and not torch.equal(st.p[k], before[k]), k


# --------------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("terms", ["l1", "reference"])
def test_training_step_loss_terms_keep_their_definitions(terms):
    """one step with A = 40 attributes beside the row: last["l1_attr"] is what the row route reports -- the mean |pred - gt| over
    the 3 + A channels of the attribute set (L1 terms alone), over the A attribute channels when the track term owns track_gs (the
    trainer's loss: L1 + D-SSIM, track, depth_loss_dpt) -- against the step's own ground-truth renderer at the start parameters
    (rtol 1e-4, as test_training_step_track_gradients_match_autograd), and every parameter group gets a gradient"""
    from test_gpu_track_loss import _step_tracks
    A, N, W, H, T, F = 40, 2500, 128, 96, 20, 3
    sc = make_scene(N, W, H, F=T, seed=11, sigma_px=3.0)
    clock = FrameClock(T)
    truth = TS.synthetic_video_params(sc, clock, "cuda", attrs=A, seed=12, cubic_sigma=0.01)
    extr = _t(sc.extr)
    start = _perturbed(truth, 3)
    t1, t2 = [0, 7, 13], [4, 2, 19]
    gt = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
    w = TS.LossWeights()
    if terms == "reference":
        gt["tracks"] = _step_tracks(gt, 4, seed=2, noise=0.5)
        w = TS.LossWeights(dssim=0.2, track=2.0, depth=0.5, depth_dpt=1.0)
    st = TS.TrainingStep(start, clock, W, H, F, extr, K=8, arap_samples=128, sample_seed=4, weights=w, spatial_order=False)
    last = st.step(t1, t2, gt)
    torch.cuda.synchronize()
    pred = TS.render_ground_truth(start, clock, W, H, extr, t1, t2)
    c0 = 3 if terms == "reference" else 0
    np.testing.assert_allclose(float(last["l1_attr"]), float((pred["attr"][:, c0:] - gt["attr"][:, c0:]).abs().mean()), rtol=1e-4)
    np.testing.assert_allclose(float(last["l1_rgb"]), float((pred["rgb"] - gt["rgb"]).abs().mean()), rtol=1e-4)
    np.testing.assert_allclose(float(last["l1_depth"]), float((pred["depth"] - gt["depth"]).abs().mean()), rtol=1e-4)
    assert np.isfinite(st.loss()) and (terms == "l1" or float(last["track"]) > 0)
    for name in TS.TRAINABLE:
        gr = st.bucket.grad(name)
        assert torch.isfinite(gr).all() and float(gr.abs().max()) > 0, name
