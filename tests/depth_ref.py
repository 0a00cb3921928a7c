"""What the depth-loss tests share (test_depth_loss_cpu.py, test_gpu_depth_loss.py): the torch restatement of the reference's
``depth_loss_dpt`` (src/loss.py:184-207), the closed-form gradient the kernels implement in float64 numpy, the project's gradient
tolerance, and the inputs of the GPU tests (so that the CPU test can show, per input, that float32 itself stays inside the loss
tolerance: the tolerance is then a property of the input, not of the kernel)."""
import numpy as np
import torch

CH = 4096          # pixels per workgroup of the depth kernels (losses.DEPTH_CHUNK; test_depth_loss_cpu.py checks it against the source)


def restate(p, g):
    """depth_loss_dpt(p, g) of one frame, in the dtype of its inputs (differentiable)"""
    t_p = torch.median(p)
    s_p = torch.mean(torch.abs(p - t_p))
    t_g = torch.median(g)
    s_g = torch.mean(torch.abs(g - t_g))
    return torch.mean(((p - t_p) / s_p - (g - t_g) / s_g) ** 2)


def restate64(p, g):
    """float64 restatement of one frame (numpy float32 in): loss, gradient w.r.t. p, (t_p, s_p, t_g, s_g), m"""
    P = torch.from_numpy(np.asarray(p, np.float64).reshape(-1)).requires_grad_(True)
    G = torch.from_numpy(np.asarray(g, np.float64).reshape(-1))
    loss = restate(P, G)
    (grad,) = torch.autograd.grad(loss, [P])
    with torch.no_grad():
        t_p, t_g = torch.median(P), torch.median(G)
        st = (float(t_p), float((P - t_p).abs().mean()), float(t_g), float((G - t_g).abs().mean()))
        m = int((P == t_p).sum())
    return float(loss.detach()), grad.numpy().reshape(np.shape(p)), st, m


def lower_median(x):
    x = np.asarray(x).reshape(-1)
    return np.partition(x, (x.size - 1) // 2)[(x.size - 1) // 2]


def closed_form(p, g):
    """loss and dL/dp of one frame by the formula of include/splat_hip.h, float64 numpy"""
    p, g = np.asarray(p, np.float64).reshape(-1), np.asarray(g, np.float64).reshape(-1)
    n = p.size
    t_p, t_g = lower_median(p), lower_median(g)
    s_p, s_g = np.abs(p - t_p).mean(), np.abs(g - t_g).mean()
    d = (p - t_p) / s_p - (g - t_g) / s_g
    a = 2.0 * d / n
    A, B = a.sum(), (a * (p - t_p)).sum()
    sg = np.sign(p - t_p)
    S, tie = sg.sum(), p == t_p
    m = tie.sum()
    grad = a / s_p - B * sg / (n * s_p ** 2) + tie / m * (-A / s_p + B * S / (n * s_p ** 2))
    return (d ** 2).mean(), grad


def assert_grad_tol(a, b, what):
    """the project's gradient tolerance, element-wise on every element: |a - b| <= 2e-3 |b| + 1e-4 max|b|"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert a.size == b.size and a.size > 0, what
    err = np.abs(a - b)
    lim = 2e-3 * np.abs(b) + 1e-4 * np.abs(b).max()
    assert (err <= lim).all(), f"{what}: {int((err > lim).sum())} of {a.size} off; worst {float((err - lim).max()):.3e}"


def assert_grad_split(got, ref, p, what):
    """assert_grad_tol on the tie set {p == median(p)} and on the other pixels separately (a tie pixel carries about n / m times
    an ordinary pixel's gradient: one call over the image would let 1e-4 max hide a 10 % error everywhere else); the non-zero
    patterns must agree"""
    got, ref, p = (np.asarray(x).reshape(-1) for x in (got, ref, p))
    tie = p == lower_median(p)
    assert tie.any(), what
    assert_grad_tol(got[tie], ref[tie], what + " (tie set)")
    if (~tie).any():
        assert_grad_tol(got[~tie], ref[~tie], what + " (other pixels)")
    assert np.array_equal(got != 0, ref != 0), what + ": non-zero pattern"


# ---------------------------------------------------------------------------------------------------- inputs of the GPU tests
def _smooth(rng, F, H, W, lo=0.2, hi=3.0):
    """a smooth ramp + noise per frame, pred and gt unrelated enough that |d| is of order 1"""
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    out = []
    for _ in range(F):
        a, b, c = rng.uniform(-1, 1, 3)
        z = a * x + b * y + c * np.sin(3 * x + 2 * y) + rng.normal(0, 0.4, (H, W))
        z = lo + (hi - lo) * (z - z.min()) / max(z.max() - z.min(), 1e-9)
        out.append(z)
    return np.stack(out)[:, None].astype(np.float32)


def _plateau(rng, H, W, frac=0.6):
    """a depth render with bg = 1.0: more than half the pixels exactly 1.0, the rest below it -- the median sits on the plateau"""
    z = _smooth(rng, 1, H, W, 0.1, 0.95)[0, 0]
    z[rng.random((H, W)) < frac] = 1.0
    return z


def inputs(name):
    """(pred, gt) float32 [F, 1, H, W] of a named case; deterministic"""
    rng = np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(name)))
    shapes = {"n1": (1, 1, 1), "n2": (1, 1, 2), "n3": (1, 3, 1), "ch-1": (1, 63, 65), "ch": (1, 64, 64), "ch+1": (1, 17, 241),
              "ragged": (1, 97, 131), "three": (3, 70, 90), "top24": (2, 37, 53), "exponents": (2, 70, 90), "signed": (2, 37, 53),
              "full": (2, 480, 854)}
    F, H, W = shapes[name]
    assert {"ch-1": CH - 1, "ch": CH, "ch+1": CH + 1}.get(name, H * W) == H * W
    gt = _smooth(rng, F, H, W)
    if name == "three":          # different medians per frame; frame 1 a plateau image
        pred = _smooth(rng, F, H, W) * np.array([0.5, 1.0, 4.0], np.float32)[:, None, None, None]
        pred[1, 0] = _plateau(rng, H, W)
    elif name == "top24":        # keys that agree in their top 24 bits: only the last digit pass decides, with many ties
        pred = (1.0 + rng.integers(0, 256, (F, 1, H, W)) * 2.0 ** -23).astype(np.float32)
    elif name == "exponents":    # keys over many exponents, both signs
        pred = (rng.choice([-1.0, 1.0], (F, 1, H, W)) * rng.uniform(1, 2, (F, 1, H, W))
                * 2.0 ** rng.integers(-20, 21, (F, 1, H, W))).astype(np.float32)
    elif name == "signed":       # both signs in pred and gt (disparity), exact zeros of both signs
        pred = rng.normal(0, 1, (F, 1, H, W)).astype(np.float32)
        gt = rng.normal(0.2, 2, (F, 1, H, W)).astype(np.float32)
        for a in (pred, gt):
            flat = a.reshape(-1)
            idx = rng.choice(flat.size, 40, replace=False)
            flat[idx[:20]] = 0.0
            flat[idx[20:]] = -0.0
    elif name == "full":         # the reference's frame size: the smooth ramp with a plateau frame
        pred = _smooth(rng, F, H, W, 0.1, 0.95)
        pred[1, 0][rng.random((H, W)) < 0.55] = 1.0
    else:
        pred = _smooth(rng, F, H, W, 0.5, 5.0)
    return pred, gt


# every case whose loss is compared at rtol 1e-5 (n1 has s = 0: non-finite by construction)
LOSS_CASES = ["n2", "n3", "ch-1", "ch", "ch+1", "ragged", "three", "top24", "exponents", "signed", "full"]
