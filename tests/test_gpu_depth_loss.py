"""The median-normalised depth loss on the GPU (losses.depth_stats / depth_dpt_loss_grad / depth_loss_dpt, csrc/loss.hip) against
the float64 restatement of the reference's ``depth_loss_dpt`` on the CPU (tests/depth_ref.py) and the reference's own vectors
(tests/golden/depth_loss.npz); the training step's depth term (LossWeights.depth_dpt, src/trainer_fragGS.py:589-601).

Medians and tie counts are compared exactly; s, the per-frame loss and the slot at rtol 1e-5 (test_depth_loss_cpu.py shows that
float32 itself keeps that on each input used here); gradients by the project's tolerance, separately on the tie set and on the
other pixels."""
import numpy as np
import pytest
import torch

import depth_ref as R
from splatter_a_video_amd import losses
from splatter_a_video_amd import train_step as TS
from test_depth_loss_cpu import GOLD

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(name):
    """per frame (loss, grad, stats, m) of a named input in float64 on the CPU; computed once, never modified"""
    if name not in _REF:
        pred, gt = R.inputs(name)
        _REF[name] = (pred, gt, [R.restate64(pred[f], gt[f]) for f in range(pred.shape[0])])
    return _REF[name]


def _run(pred, gt, scale=1.0, grad=None, accumulate=False, gt_stats=None, want_grad=True):
    """every output of one call on device tensors pred, gt [F, 1, H, W]"""
    F = pred.shape[0]
    if grad is None and want_grad:
        grad = torch.full(pred.shape, float("nan"), device="cuda")          # written in full: no NaN may survive
    per = torch.empty(F, device="cuda")
    slot = torch.full((1,), 0.25, device="cuda")                            # the slot is added to
    stats = torch.empty(F, 4, device="cuda")
    ties = torch.empty(F, dtype=torch.int32, device="cuda")
    losses.depth_dpt_loss_grad(pred, gt, scale, grad, accumulate=accumulate, per_frame=per, loss_slot=slot, gt_stats=gt_stats,
                               stats=stats, ties=ties)
    torch.cuda.synchronize()
    return dict(grad=grad, per=per, slot=slot, stats=stats, ties=ties)


def _check(name, out, pred, gt, ref, scale=1.0, base=None):
    F = pred.shape[0]
    st = out["stats"].cpu().numpy()
    per = out["per"].cpu().numpy()
    for f in range(F):
        loss, grad, (tp, sp, tg, sg), m = ref[f]
        # the medians and the tie count are exact
        assert float(st[f, 0]) == float(torch.median(torch.from_numpy(pred[f]))) == tp, (name, f)
        assert float(st[f, 2]) == float(torch.median(torch.from_numpy(gt[f]))) == tg, (name, f)
        assert int(out["ties"][f]) == m, (name, f)
        np.testing.assert_allclose(st[f, 1], sp, rtol=1e-5, err_msg=f"{name} s_p {f}")
        np.testing.assert_allclose(st[f, 3], sg, rtol=1e-5, err_msg=f"{name} s_g {f}")
        np.testing.assert_allclose(per[f], loss, rtol=1e-5, err_msg=f"{name} loss {f}")
        if out["grad"] is not None:
            got = out["grad"][f, 0].cpu().numpy().astype(np.float64)
            if base is not None:
                got = got - base[f, 0].astype(np.float64)
            if pred[f].size == 2:
                # two pixels normalise to (0, 2) whatever their values: the loss does not depend on p, the true gradient is
                # exactly 0 and both results are rounding residue of terms of size T = 2 max|d| / (n s_p) -- a relative
                # tolerance means nothing; float32 keeps the residue far below 1e-5 T
                T = scale / F * 2.0 * np.sqrt(2.0 * loss) / (2.0 * sp)
                assert np.abs(scale / F * grad).max() <= 1e-12 * T and np.abs(got).max() <= 1e-5 * T, (name, got, T)
                continue
            R.assert_grad_split(got, scale / F * grad, pred[f], f"{name} frame {f}")
    np.testing.assert_allclose(float(out["slot"]) - 0.25, np.mean([r[0] for r in ref]), rtol=1e-5, atol=2e-7)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ["n2", "n3", "ch-1", "ch", "ch+1", "ragged", "three", "top24", "exponents", "signed"])
def test_loss_stats_and_gradient_against_float64(name):
    pred, gt, ref = _reference(name)
    out = _run(_dev(pred), _dev(gt), scale=1.5)
    _check(name, out, pred, gt, ref, scale=1.5)
    if name == "three":          # different medians per frame, frame 1 on its plateau
        assert len({r[2][0] for r in ref}) == 3 and ref[1][2][0] == 1.0 and ref[1][3] > 1000
    if name == "top24":          # only the last digit decides, and it decides among ties
        assert all(r[3] > 1 for r in ref)


def test_a_single_pixel_has_zero_scale():
    """n = 1: s = 0, the reference's loss is 0 / 0; the call succeeds and gives a non-finite loss too"""
    pred, gt = R.inputs("n1")
    assert not np.isfinite(R.restate64(pred[0], gt[0])[0])
    out = _run(_dev(pred), _dev(gt))
    assert not np.isfinite(float(out["per"][0]))
    assert float(out["stats"][0, 0]) == float(pred.reshape(-1)[0]) and float(out["stats"][0, 1]) == 0.0


def test_full_size_frames():
    """2 x 480 x 854: grid and size arithmetic at the reference's frame size"""
    pred, gt, ref = _reference("full")
    for f in range(2):
        assert ref[f][2][0] == R.lower_median(pred[f]) and ref[f][2][2] == R.lower_median(gt[f])
    out = _run(_dev(pred), _dev(gt))
    _check("full", out, pred, gt, ref)
    assert int(out["ties"][1]) > 100000


def test_strided_pred_and_grad_and_accumulate():
    """pred a channel slice of a wider row, gt transposed storage, grad a channel slice of a non-zero image, added to"""
    pred, gt, ref = _reference("three")
    F, _, H, W = pred.shape
    wide = torch.randn(F, 4, H, W, device="cuda")
    wide[:, 2] = _dev(pred)[:, 0]
    g_t = _dev(gt).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)          # column-major planes
    assert not g_t.is_contiguous()
    # (a non-zero image of the gradient's own magnitude: base + g is rounded to float32 once, and on a base of order 1 that
    #  rounding alone, 6e-8, would be as large as the tolerance of a gradient of order 1e-4)
    gwide = 1e-4 * torch.randn(F, 3, H, W, device="cuda")
    before = gwide.clone()
    out = _run(wide[:, 2:3], g_t, scale=0.7, grad=gwide[:, 1:2], accumulate=True)
    _check("strided", out, pred, gt, ref, scale=0.7, base=before[:, 1:2].cpu().numpy())
    assert torch.equal(gwide[:, 0], before[:, 0]) and torch.equal(gwide[:, 2], before[:, 2])
    assert torch.equal(wide[:, 2], _dev(pred)[:, 0])
    # written, not added: the same values as a contiguous call's, bit for bit
    plain = _run(_dev(pred), _dev(gt), scale=0.7)
    gw2 = torch.full((F, 3, H, W), 5.0, device="cuda")
    out2 = _run(wide[:, 2:3], g_t, scale=0.7, grad=gw2[:, 1:2])
    assert torch.equal(out2["grad"], plain["grad"]) and torch.equal(out2["per"], plain["per"])
    assert bool((gw2[:, 0] == 5.0).all()) and bool((gw2[:, 2] == 5.0).all())
    # planes that start off a 16-byte boundary (37 x 53 floats per plane): the same bits as the aligned call's
    pred, gt, ref = _reference("signed")
    F, _, H, W = pred.shape
    assert (H * W) % 4 != 0
    wide = torch.randn(F, 4, H, W, device="cuda")
    wide[:, 1] = _dev(pred)[:, 0]
    gw3 = torch.zeros(F, 3, H, W, device="cuda")
    out3 = _run(wide[:, 1:2], _dev(gt), grad=gw3[:, 1:2])
    _check("unaligned", out3, pred, gt, ref)
    plain = _run(_dev(pred), _dev(gt))
    for k in plain:
        assert torch.equal(out3[k], plain[k]), k


def test_cached_gt_stats_give_the_same_bits():
    pred, gt, ref = _reference("three")
    p, g = _dev(pred), _dev(gt)
    gs = losses.depth_stats(g)
    a, b = _run(p, g), _run(p, g, gt_stats=gs)
    assert torch.equal(gs, a["stats"][:, 2:])
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for f in range(3):
        assert float(gs[f, 0]) == ref[f][2][2]
        np.testing.assert_allclose(float(gs[f, 1]), ref[f][2][3], rtol=1e-5)
    # depth_stats of the strided pred slice
    wide = torch.randn(3, 4, *pred.shape[2:], device="cuda")
    wide[:, 1] = p[:, 0]
    assert torch.equal(losses.depth_stats(wide[:, 1:2]), a["stats"][:, :2])


def test_a_nan_poisons_its_frame_only():
    pred, gt, _ = _reference("three")
    p, g = _dev(pred), _dev(gt)
    clean = _run(p, g)
    for where in ("pred", "gt"):
        p2, g2 = p.clone(), g.clone()
        (p2 if where == "pred" else g2)[1, 0, 11, 17] = float("nan")
        out = _run(p2, g2)
        assert bool(torch.isnan(out["per"][1])) and bool(torch.isnan(out["grad"][1]).all()), where
        assert bool(torch.isnan(out["slot"]))
        for f in (0, 2):
            assert torch.equal(out["per"][f], clean["per"][f]) and torch.equal(out["grad"][f], clean["grad"][f]), (where, f)
            assert torch.equal(out["stats"][f], clean["stats"][f]) and torch.equal(out["ties"][f], clean["ties"][f])


@pytest.mark.parametrize("name", ["three", "full"])
def test_two_runs_are_bit_equal(name):
    pred, gt, _ = _reference(name)
    p, g = _dev(pred), _dev(gt)
    a, b = _run(p, g), _run(p, g)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the loss alone (no gradient image): the same numbers
    c = _run(p, g, want_grad=False)
    assert c["grad"] is None
    for k in ("per", "slot", "stats", "ties"):
        assert torch.equal(a[k], c[k]), k


@pytest.mark.parametrize("case", ["smooth", "plateau", "odd", "signed", "nan"])
def test_autograd_function_against_the_reference_fixture(case):
    """losses.depth_loss_dpt in the trainer's call shape [H, W, 1] against the reference's own values and gradients"""
    g = np.load(GOLD)
    pred, gt = g[f"{case}_pred"], g[f"{case}_gt"]
    p = _dev(pred)[..., None].requires_grad_(True)
    loss = losses.depth_loss_dpt(p, _dev(gt)[..., None])
    (grad,) = torch.autograd.grad(3.0 * loss, [p])
    assert grad.shape == p.shape and loss.dim() == 0
    grad = grad[..., 0].cpu().numpy()
    if case == "nan":
        assert np.isnan(float(loss)) and np.isnan(grad).all()
        return
    np.testing.assert_allclose(float(loss), float(g[f"{case}_loss"]), rtol=1e-5)
    R.assert_grad_split(grad, 3.0 * g[f"{case}_grad"].astype(np.float64), pred, case)
    want_loss, want, _, _ = R.restate64(pred, gt)
    np.testing.assert_allclose(float(loss), want_loss, rtol=1e-5)
    R.assert_grad_split(grad, 3.0 * want, pred, case + " (float64)")


def test_autograd_function_shapes():
    """[F, 1, H, W]: the mean over the frames; any other shape: one frame of numel pixels; strided views; refusals"""
    pred, gt, ref = _reference("three")
    p, g = _dev(pred).requires_grad_(True), _dev(gt)
    loss = losses.depth_loss_dpt(p, g)
    np.testing.assert_allclose(float(loss), np.mean([r[0] for r in ref]), rtol=1e-5)
    (grad,) = torch.autograd.grad(loss, [p])
    for f in range(3):
        R.assert_grad_split(grad[f, 0].cpu().numpy(), ref[f][1] / 3, pred[f], f"frame {f}")
    # [3, H, W] is ONE frame of 3 H W pixels
    one = losses.depth_loss_dpt(p.detach()[:, 0], g[:, 0])
    want = R.restate64(pred[:, 0], gt[:, 0])[0]
    np.testing.assert_allclose(float(one), want, rtol=1e-5)
    # out[1] of a render: a [F, 1, H, W] slice of a wider row, differentiated through the slice
    wide = torch.randn(3, 4, *pred.shape[2:], device="cuda")
    wide[:, 3] = p.detach()[:, 0]
    wide.requires_grad_(True)
    l2 = losses.depth_loss_dpt(wide[:, 3:4], g)
    (gw,) = torch.autograd.grad(l2, [wide])
    assert torch.equal(l2, loss) and torch.equal(gw[:, 3:4], grad) and not bool(gw[:, :3].any())
    with pytest.raises(NotImplementedError):
        losses.depth_loss_dpt(p, g, weight=g)
    with pytest.raises(ValueError):
        losses.depth_loss_dpt(p, g[:2])
    with pytest.raises(ValueError):
        losses.depth_loss_dpt(p, g.clone().requires_grad_(True))


# ------------------------------------------------------------------------------------------------------------ training step
class _Capture(TS.TrainingStep):
    """keeps the rendered depth the depth term saw and the gradient image it handed to the blend backward"""

    def _depth_loss_grad(self, pred, gt, sums, slot):
        self.seen_pred = pred.detach().clone()
        g = super()._depth_loss_grad(pred, gt, sums, slot)
        self.seen_grad = g.clone()
        return g


def _step_setup():
    from test_gpu_train_step import _clip, _perturbed, _t
    N, W, H, T, F = 3000, 128, 96, 20, 4
    sc, clock, truth = _clip(N, W, H, T, seed=9)
    extr = _t(sc.extr)
    t1, t2 = [0, 3, 7, 12], [5, 1, 19, 2]
    gt = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
    # a monocular prior: a depth map up to an unknown scale and shift, plus noise
    gen = torch.Generator(device="cuda").manual_seed(5)
    # (of the mirrored neighbouring frame: pred and gt must not be near-identical after normalisation, or the loss is a
    #  difference of nearly equal numbers and float32 itself leaves the loss tolerance)
    gt["depth"] = (3.0 * gt["depth"].roll(1, 0).flip(-1) - 0.5
                   + 0.2 * torch.randn(gt["depth"].shape, device="cuda", generator=gen)).contiguous()
    make = lambda cls, w: cls(_perturbed(truth, 3), clock, W, H, F, extr, K=8, arap_samples=128, sample_seed=4, weights=w)
    return make, t1, t2, gt, (F, H, W)


def test_training_step_depth_term():
    make, t1, t2, gt, (F, H, W) = _step_setup()
    st = make(_Capture, TS.LossWeights(depth=0.0, depth_dpt=1.0))
    last = st.step(t1, t2, gt)
    torch.cuda.synchronize()
    assert set(last) == {"l1_rgb", "l1_depth", "l1_attr", "arap", "depth_dpt"}
    assert float(last["l1_depth"]) == 0.0          # no L1 on depth at depth = 0
    pred = st.seen_pred
    assert pred.shape == (F, 1, H, W)
    # by hand on the step's own rendered depth
    grad = torch.empty(F, 1, H, W, device="cuda")
    per = torch.empty(F, device="cuda")
    losses.depth_dpt_loss_grad(pred, gt["depth"], 1.0, grad, per_frame=per)
    assert torch.equal(st.seen_grad, grad)
    np.testing.assert_allclose(float(last["depth_dpt"]), float(per.double().mean()), rtol=1e-6)
    # ... which is the float64 restatement's
    pn, gn = pred.cpu().numpy(), gt["depth"].cpu().numpy()
    for f in range(F):
        loss, g64, _, m = R.restate64(pn[f], gn[f])
        np.testing.assert_allclose(float(per[f]), loss, rtol=1e-5)
        R.assert_grad_split(grad[f].cpu().numpy(), g64 / F, pn[f], f"step frame {f}")
    for name in ("pos_cubic_node", "rotation", "opacity", "scaling"):
        assert float(st.bucket.grad(name).abs().max()) > 0, name
    assert abs(st.loss() - (float(last["l1_rgb"]) + float(last["l1_attr"]) + 1e-3 * float(last["arap"])
                            + float(last["depth_dpt"]))) <= 1e-6 * max(1.0, abs(st.loss()))
    # cached ground-truth statistics: the same step, bit for bit
    st2 = make(_Capture, TS.LossWeights(depth=0.0, depth_dpt=1.0))
    last2 = st2.step(t1, t2, dict(gt, depth_stats=losses.depth_stats(gt["depth"])))
    assert torch.equal(st2.seen_grad, st.seen_grad) and torch.equal(last2["depth_dpt"], last["depth_dpt"])
    # both depth terms: the L1's gradient image + depth_dpt * the new term's
    st3 = make(_Capture, TS.LossWeights(depth=0.5, depth_dpt=2.0))
    last3 = st3.step(t1, t2, gt)
    assert torch.equal(st3.seen_pred, pred)
    both = 0.5 / (F * H * W) * torch.sign(pred - gt["depth"])
    losses.depth_dpt_loss_grad(pred, gt["depth"], 2.0, both, accumulate=True)
    R.assert_grad_tol(st3.seen_grad.cpu().numpy(), both.cpu().numpy(), "both depth terms")
    np.testing.assert_allclose(float(last3["l1_depth"]), float((pred - gt["depth"]).abs().mean()), rtol=1e-4)
    assert torch.equal(last3["depth_dpt"], last["depth_dpt"])


def test_training_step_off_switch():
    """depth_dpt = 0.0: the parameters after two steps are those of a step object built without the field set, bit for bit"""
    make, t1, t2, gt, _ = _step_setup()
    a = make(TS.TrainingStep, TS.LossWeights(depth_dpt=0.0))
    b = make(TS.TrainingStep, None)
    for st in (a, b):
        for _ in range(2):
            last = st.step(t1, t2, gt)
        assert "depth_dpt" not in last
    torch.cuda.synchronize()
    assert torch.equal(a.bucket.flat_param, b.bucket.flat_param)
    assert float(a.bucket.flat_param.abs().max()) > 0
