"""SSIM / D-SSIM on the GPU (splatter_a_video_amd/losses.py, csrc/loss.hip) against a float64 restatement of the reference's
`_ssim` (src/pointrix/model/loss.py:58-112, grouped conv2d with the 11 x 11 window; written here, not copied), and the training
step's L1 + D-SSIM RGB term (LossWeights.dssim, src/trainer_fragGS.py:575-578)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from splatter_a_video_amd import losses
from splatter_a_video_amd import train_step as TS
from test_gpu_train_step import _clip, _perturbed, _t

pytestmark = pytest.mark.gpu


def ref_ssim(img1, img2, window_size=11, size_average=True):
    """the reference's ssim: channel = dim -3, grouped 2-D correlation with the normalised Gaussian outer product (sigma 1.5),
    zero padding window_size // 2; in the inputs' dtype and device"""
    C = img1.shape[-3]
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / (2 * 1.5 ** 2)) for x in range(window_size)], dtype=torch.float64)
    g = g / g.sum()
    w = (g[:, None] @ g[None, :]).to(img1.dtype).to(img1.device).expand(C, 1, window_size, window_size).contiguous()
    conv = lambda t: Fn.conv2d(t, w, padding=window_size // 2, groups=C)
    mu1, mu2 = conv(img1), conv(img2)
    s1 = conv(img1 * img1) - mu1 ** 2
    s2 = conv(img2 * img2) - mu2 ** 2
    s12 = conv(img1 * img2) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def _pair(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    gt = torch.rand(shape, device="cuda", generator=g)
    pred = (gt + 0.15 * torch.randn(shape, device="cuda", generator=g)).clamp(0, 1)
    return pred, gt


def _cpu64(t):
    return t.detach().cpu().double()


def assert_grad_tol(a, b, what):
    """the project's gradient tolerance, element-wise on every element: |a - b| <= 2e-3 |b| + 1e-4 max|b|"""
    a, b = _cpu64(a).numpy().reshape(-1), _cpu64(b).numpy().reshape(-1)
    err = np.abs(a - b)
    lim = 2e-3 * np.abs(b) + 1e-4 * np.abs(b).max()
    assert (err <= lim).all(), f"{what}: {int((err > lim).sum())} of {a.size} off; worst {float((err - lim).max()):.3e}"


# (name, the [N, Cp, Hp, Wp] view of a fresh tensor, window)
def _case(name):
    if name == "image":
        return _pair((2, 3, 480, 854), 1)
    if name == "reference":          # the trainer's literal call: the HWC view of [F, 3, H, W] frames, planes of W x 3
        p, g = _pair((2, 3, 480, 854), 2)
        return p.permute(0, 2, 3, 1), g.permute(0, 2, 3, 1)
    if name == "image_s":
        return _pair((2, 3, 120, 214), 4)
    if name == "reference_s":
        p, g = _pair((2, 3, 120, 214), 5)
        return p.permute(0, 2, 3, 1), g.permute(0, 2, 3, 1)
    shape = {"1x1": (2, 3, 1, 1), "5x3": (2, 4, 5, 3), "37x61": (2, 3, 37, 61), "small_plane": (3, 2, 6, 4)}[name]
    return _pair(shape, 3)


CASES = ["image", "reference", "1x1", "5x3", "37x61", "small_plane"]


@pytest.mark.parametrize("window", [11, 7])
@pytest.mark.parametrize("name", CASES)
def test_ssim_value(name, window):
    a, b = _case(name)
    if name == "reference":
        assert not a.is_contiguous()
    for size_average in (True, False):
        got = losses.ssim(a, b, window, size_average)
        want = ref_ssim(_cpu64(a), _cpu64(b), window, size_average)
        assert got.shape == want.shape
        assert float((_cpu64(got) - want).abs().max()) <= 1e-5, (name, window, size_average, got, want)
    if a.shape[0] == 1 or name == "37x61":     # [C, H, W] with size_average=True
        got = losses.ssim(a[0], b[0], window)
        assert abs(float(got) - float(ref_ssim(_cpu64(a[0]), _cpu64(b[0]), window))) <= 1e-5


@pytest.mark.parametrize("window", [11, 7])
@pytest.mark.parametrize("name", ["image_s", "reference_s", "5x3", "37x61", "small_plane"])
def test_ssim_gradients(name, window):
    a0, b0 = _case(name)
    for size_average in (True, False):
        a, b = a0.detach().requires_grad_(True), b0.detach().requires_grad_(True)
        s = losses.ssim(a, b, window, size_average)
        up = torch.linspace(0.5, 1.5, s.numel(), device="cuda").reshape(s.shape)
        ga, gb = torch.autograd.grad((s * up).sum(), [a, b])
        ra, rb = _cpu64(a0).requires_grad_(True), _cpu64(b0).requires_grad_(True)
        sr = ref_ssim(ra, rb, window, size_average)
        wa, wb = torch.autograd.grad((sr * _cpu64(up)).sum(), [ra, rb])
        assert ga.shape == a.shape and gb.shape == b.shape
        assert_grad_tol(ga, wa, f"{name} img1")
        assert_grad_tol(gb, wb, f"{name} img2")


def test_restatement_passes_gradcheck():
    """validates the test itself: the float64 restatement's autograd against finite differences"""
    g = torch.Generator().manual_seed(0)
    a = torch.rand(1, 2, 7, 9, dtype=torch.float64, generator=g, requires_grad=True)
    b = torch.rand(1, 2, 7, 9, dtype=torch.float64, generator=g, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x, y: ref_ssim(x, y, 5), (a, b))


def test_single_gradient_and_double_backward():
    a, b = _pair((1, 3, 40, 50), 5)
    a.requires_grad_(True)
    s = losses.ssim(a, b)
    (ga,) = torch.autograd.grad(s, [a], create_graph=True)
    with pytest.raises(RuntimeError):
        ga.sum().backward()


def test_channel_slice_of_a_wider_row_is_read_in_place():
    """the RGB slice of a composited [F, 23, H, W] row (and its HWC view) gives the bits of its contiguous copy"""
    g = torch.Generator(device="cuda").manual_seed(9)
    row = torch.rand(3, 23, 96, 128, device="cuda", generator=g)
    gt = torch.rand(3, 3, 96, 128, device="cuda", generator=g)
    for view in (lambda t: t, lambda t: t.permute(0, 2, 3, 1)):
        sl = row[:, 0:3].detach().requires_grad_(True)
        cp = row[:, 0:3].contiguous().requires_grad_(True)
        outs = []
        for x in (sl, cp):
            s = losses.ssim(view(x), view(gt), 11, False)
            (gx,) = torch.autograd.grad(s.sum(), [x])
            outs.append((s, gx))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        d = losses.dssim_l1(row[:, 0:3], gt, 0.2, "image")
        assert torch.equal(d, losses.dssim_l1(row[:, 0:3].contiguous(), gt, 0.2, "image"))


def test_determinism_and_graph_capture():
    """no float atomics: two runs give the same bits; forward + backward captured by torch.cuda.graph replay to them"""
    a0, b = _pair((2, 3, 96, 128), 11)
    a = a0.clone().requires_grad_(True)

    def run():
        s = losses.ssim(a, b)
        (g,) = torch.autograd.grad(s, [a])
        d = losses.dssim_l1(a.detach(), b, 0.2, "reference")
        return s.detach(), g, d

    r1, r2 = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(static, r1))


@pytest.mark.parametrize("layout", ["reference", "image"])
def test_dssim_l1_value_and_gradient(layout):
    lam = 0.2
    pred0, gt = _pair((3, 3, 120, 214), 13)
    pred = pred0.clone().requires_grad_(True)
    loss = losses.dssim_l1(pred, gt, lam, layout)
    (g,) = torch.autograd.grad(loss * 1.7, [pred])
    rp = _cpu64(pred0).requires_grad_(True)
    rg = _cpu64(gt)
    view = (lambda t: t.permute(0, 2, 3, 1)) if layout == "reference" else (lambda t: t)
    want = (1 - lam) * (rp - rg).abs().mean() + lam * (1 - ref_ssim(view(rp), view(rg)))
    (wg,) = torch.autograd.grad(want * 1.7, [rp])
    assert abs(float(loss.detach()) - float(want)) <= 1e-5
    assert_grad_tol(g, wg, f"dssim_l1 {layout}")
    with pytest.raises(ValueError):
        losses.dssim_l1(pred, gt.requires_grad_(True), lam, layout)


class _AutogradRGB(TS.TrainingStep):
    """the RGB term's gradient by torch autograd through the restatement (float32 on the GPU)"""

    def _rgb_loss_grad(self, pred, target, sums):
        p = pred.detach().clone().requires_grad_(True)
        lam = self.w.dssim
        view = (lambda t: t.permute(0, 2, 3, 1)) if self.w.ssim_layout == "reference" else (lambda t: t)
        s = ref_ssim(view(p), view(target))
        loss = self.w.rgb * ((1 - lam) * (p - target).abs().mean() + lam * (1 - s))
        (g,) = torch.autograd.grad(loss, [p])
        sums[0] += (p - target).abs().sum().detach()
        sums[3] += s.detach() * p.numel()
        return g.contiguous()


@pytest.mark.parametrize("layout", ["reference", "image"])
def test_training_step_dssim_gradients_match_autograd(layout):
    N, W, H, T, F = 3000, 128, 96, 20, 4
    sc, clock, truth = _clip(N, W, H, T, seed=11)
    extr = _t(sc.extr)
    start = _perturbed(truth, 3)
    t1, t2 = [0, 3, 7, 12], [5, 1, 19, 2]
    gt = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
    w = TS.LossWeights(dssim=0.2, ssim_layout=layout)
    res = []
    for cls in (TS.TrainingStep, _AutogradRGB):
        st = cls(start, clock, W, H, F, extr, K=8, arap_samples=128, sample_seed=4, weights=w)
        last = st.step(t1, t2, gt)
        torch.cuda.synchronize()
        res.append((st, last))
    (a, la), (b, lb) = res
    assert set(la) == {"l1_rgb", "l1_depth", "l1_attr", "arap", "ssim_rgb"}
    for name in ("pos_cubic_node", "rotation", "opacity", "scaling", "shs", "attrs"):
        assert float(a.bucket.grad(name).abs().max()) > 0, name
        assert_grad_tol(a.bucket.grad(name), b.bucket.grad(name), name)
    # the step's SSIM = the restatement on the images it rendered: re-render the start parameters' frames
    pred = TS.render_ground_truth({k: v for k, v in start.items()}, clock, W, H, extr, t1, t2)["rgb"]
    view = (lambda t: t.permute(0, 2, 3, 1)) if layout == "reference" else (lambda t: t)
    want = float(ref_ssim(_cpu64(view(pred)), _cpu64(view(gt["rgb"]))))
    assert abs(float(la["ssim_rgb"]) - want) <= 1e-5, (float(la["ssim_rgb"]), want)
    assert abs(float(lb["ssim_rgb"]) - want) <= 1e-5


def test_training_step_with_dssim_converges():
    N, W, H, T, F = 4000, 128, 96, 20, 5
    sc, clock, truth = _clip(N, W, H, T, seed=5)
    extr = _t(sc.extr)
    rng = np.random.default_rng(0)
    lr = dict(TS.REFERENCE_LR, pos_cubic_node=2e-3, shs=2e-2, attrs=2e-2, scaling=1e-2, rotation=5e-3)
    st = TS.TrainingStep(_perturbed(truth, 1), clock, W, H, F, extr, lr=lr, K=8, arap_samples=256,
                         weights=TS.LossWeights(dssim=0.2))
    gts = {}
    losses_, ssims = [], []
    for it in range(150):
        t1 = [int(t) for t in rng.choice(T, F, replace=False)]
        t2 = [int(rng.choice([t for t in range(T) if t != x])) for x in t1]
        key = (tuple(t1), tuple(t2))
        if key not in gts:
            gts[key] = TS.render_ground_truth(truth, clock, W, H, extr, t1, t2)
        last = st.step(t1, t2, gts[key])
        losses_.append(st.loss())
        ssims.append(float(last["ssim_rgb"]))
    assert all(np.isfinite(losses_))
    first, final = float(np.mean(losses_[:3])), float(np.mean(losses_[-5:]))
    assert final < first / 3.0, (first, final)
    assert np.mean(ssims[-5:]) > np.mean(ssims[:3]), (ssims[:3], ssims[-5:])
