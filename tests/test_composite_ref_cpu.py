"""tests/composite_ref.py on the CPU: the float64 reference of the compositing kernels is right, its scenes are decision-clear,
and its error bars are attainable by float32 arithmetic of the kernels' form.

  * the analytic backward agrees with torch.autograd through torch_twin.blend in float64 (rtol 1e-9 per element), the forward's
    image, ncontrib and gs_idx with torch_twin.blend: 48 x 32, 200 Gaussians, C = 3, with and without a bias;
  * prune() reaches a fixed point on every scene and removes at most 5 % of the Gaussians; the coverage the GPU tests rely on
    holds after pruning;
  * a numpy float32 restatement of the kernels' arithmetic (composite_ref.f32_forward_backward) makes every decision of the
    float64 walk on the pruned scenes; its worst error / companion ratio per output (K = 1) is measured, and each K is the
    smallest power of two at or above 4 x that ratio -- the factor 4 for what the restatement cannot show (v_exp_f32 and
    v_log_f32 are not correctly rounded, the fma emulation rounds twice, the kernels' summation orders differ).  The ratios,
    the K values and the pruned counts are recorded in profiles/composite_reference_cpu_float32.json and re-checked here:
    the measured ratios must still be covered by the recorded K (4 x ratio <= K), and K must be what the recorded ratio gives
    (tools/composite_reference_report.py --backend float32 writes the file).
    The C oracle is not used to set K: it evaluates the reference's direct form of `power`."""
import json
import math
import os

import numpy as np
import pytest
import torch

import composite_ref as cr
import torch_twin as tw
from splatter_a_video_amd.synth import make_scene
from test_gpu_parity import oracle_geometry

PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "composite_reference_cpu_float32.json")
SCENES = ("opaque_100x60", "opaque_100x60_bias", "hard_64x48")
OUTPUTS = ("image", "final_T") + cr.GRADS
# (scene, C, K of the id lists, truncation): the restatement's cases
CASES = [("opaque_100x60", 3, 20, False), ("opaque_100x60", 3, 2, True), ("opaque_100x60", 33, 0, False),
         ("opaque_100x60_bias", 3, 0, False), ("hard_64x48", 3, 0, False)]
BG = 0.3


def pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(x))


def case_inputs(sc, C):
    """the seeded features and upstream gradient of a (scene, C) case: shared with the GPU tests"""
    rng = np.random.default_rng(1000 + C)
    return rng.uniform(size=(sc.N, C)).astype(np.float32), rng.normal(size=(C, sc.H, sc.W)).astype(np.float32)


@pytest.mark.parametrize("with_bias", [False, True])
def test_reference_matches_twin_and_autograd(oracle_mod, with_bias):
    N, W, H, C, K = 200, 48, 32, 3, 4
    sc = make_scene(N, W, H, seed=3)
    G = oracle_geometry(oracle_mod, sc)
    rng = np.random.default_rng(4)
    feat = rng.uniform(size=(N, C))
    g = rng.normal(size=(C, H, W))
    bias = rng.uniform(-0.05, 0.1, size=(N, 1)) if with_bias else None
    wk = cr.walk(G["uv"], G["conic"], sc.opacity, G["idx"], G["tr"], W, H, bias=bias, K=K)
    img, _ = cr.forward(wk, feat, BG)
    fT, nc, gi = wk.image_maps()
    grads, _ = cr.backward(wk, G["conic"], sc.opacity, feat, BG, g)

    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in
         dict(uv=G["uv"], conic=G["conic"], opacity=sc.opacity, feature=feat).items()}
    tb = torch.tensor(bias, requires_grad=True) if with_bias else None
    out, fT_t, nc_t, gi_t = tw.blend(t["uv"], t["conic"], t["opacity"], t["feature"], G["idx"], G["tr"], BG, W, H, bias=tb, K=K)
    assert int((nc_t > 0).sum()) > 0.5 * W * H and int((gi_t >= 0).sum()) > 0
    np.testing.assert_allclose(img, out.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(fT, fT_t.numpy(), rtol=1e-12)
    assert np.array_equal(nc, nc_t.numpy()) and np.array_equal(gi, gi_t.numpy())
    (out * torch.tensor(g)).sum().backward()
    for name in ("uv", "conic", "opacity", "feature"):
        ref = t[name].grad.numpy().reshape(grads[name].shape)
        assert np.abs(ref).max() > 0
        np.testing.assert_allclose(grads[name], ref, rtol=1e-9, atol=0, err_msg=name)
    if with_bias:
        np.testing.assert_allclose(grads["bias"], tb.grad.numpy().reshape(-1), rtol=1e-9, atol=0)
    # |d uv|: one chunk of channels and an upstream gradient of one sign per pixel's dL/dalpha is not available from autograd;
    # the sums of magnitudes bound the signed ones, element by element
    assert (grads["abs_uv"] >= np.abs(grads["uv"]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("name", SCENES)
def test_prune_reaches_a_fixed_point_and_keeps_the_coverage(oracle_mod, name):
    sc = cr.scene(oracle_mod, name)
    rec = json.load(open(PROFILE))["scenes"][name]
    assert sc.passes[-1] == 0 and sum(sc.passes) == sc.pruned.size
    assert sc.pruned.size <= 0.05 * sc.N, f"{name}: pruned {sc.pruned.size} of {sc.N}"
    assert (sc.radius.reshape(-1)[sc.pruned] == 0).all() and not np.isin(sc.pruned, sc.idx).any()
    wk = cr.scene_walk(sc)
    assert wk.unclear_ids().size == 0
    cov = cr.coverage(sc, wk)
    print(name, "pruned", sc.pruned.size, "of", sc.N, "passes", sc.passes, "evaluations", wk.evaluations(), "M max", wk.Mmax(),
          {k: v for k, v in cov.items() if k != "lengths"})
    assert rec["pruned"] == int(sc.pruned.size) and rec["passes"] == [int(p) for p in sc.passes] and rec["N"] == sc.N
    n = cov["lengths"]
    if name.startswith("opaque"):
        assert sc.W % 16 and sc.H % 16, "partial tiles in both directions"
        assert cov["empty"] >= 1 and sc.culled.size > 0, "an empty tile, its reaching Gaussians culled"
        assert cov["stopped_pixels"] > 0, "pixels that stop before their list ends"
        assert cov["saturated_tiles"], "a tile that saturates entirely"
        assert n.max() > 256
        # 18 applied entries of one quarter within 64 consecutive list positions: applied entries at positions 0, 1, 15, 16 and 17
        # of a quarter list, whichever way a kernel stages the list
        assert cov["quarter_applied_64"] >= 18
        if sc.bias is None:
            assert cov["long_to_end"], "a list longer than 256 entries walked to its end"
    else:
        ids = np.arange(150, 166)
        mid = any(e - b >= 3 and np.isin(sc.idx[b + 1:e - 1], ids).any() for b, e in sc.tr)
        assert mid, "a NaN / inf entry in mid-list"
        assert np.isin(np.arange(60, 100), sc.idx).sum() >= 38 and float(np.abs(sc.conic[60:100]).max()) > 1e4, "the needles stay"
        applied = np.zeros(sc.N, bool)
        for t in wk.tiles:
            applied[t.ids[t.applied.any(1)]] = True
        assert applied[60:100].sum() >= 10, "needles that apply to a pixel"
        assert not applied[0:20].any() and not applied[150:166].any(), "opacity 0 / 1e-30 and non-finite rows apply nowhere"
        assert applied[20:60].any() and not applied[20:60].all(), "centre alphas on both sides of 1/255"


def measure(o):
    """worst |float32 restatement - float64| / companion per output over CASES (and that every decision agrees)"""
    worst = {k: 0.0 for k in OUTPUTS}
    for name, C, K, trunc in CASES:
        sc = cr.scene(o, name)
        wk = cr.scene_walk(sc, K, trunc)
        assert wk.unclear_ids().size == 0, (name, K, trunc)
        feat, g = case_inputs(sc, C)
        img, cimg = cr.forward(wk, feat, BG)
        fT, nc, gi = wk.image_maps()
        grads, comps = cr.backward(wk, sc.conic, sc.opacity, feat, BG, g)
        r = cr.f32_forward_backward(sc.uv, sc.conic, sc.opacity, feat, sc.idx, sc.tr, BG, sc.W, sc.H, g, bias=sc.bias, K=K, truncate=trunc)
        assert np.array_equal(r["ncontrib"], nc), f"{name}: ncontrib"
        assert np.array_equal(r["gs_idx"], gi), f"{name}: gs_idx"
        for a, t in zip(r["applied"], wk.tiles):
            assert np.array_equal(a[:t.ids.size], t.applied) and not a[t.ids.size:].any(), f"{name}: applied structure of tile {t.tile}"
        ratios = dict(image=cr.worst_ratio(r["image"], img, cimg), final_T=cr.worst_ratio(r["final_T"], fT, wk.final_T_companion()))
        for k in cr.GRADS:
            if k == "bias" and sc.bias is None:
                continue
            assert np.isfinite(r["grads"][k]).all() and np.abs(grads[k]).max() > 0
            ratios[k] = cr.worst_ratio(r["grads"][k], grads[k], comps[k])
        print(name, C, K, trunc, {k: round(v, 4) for k, v in ratios.items()})
        for k, v in ratios.items():
            worst[k] = max(worst[k], v)
    return worst


def test_float32_restatement_attains_the_bars(oracle_mod):
    rec = json.load(open(PROFILE))
    worst = measure(oracle_mod)
    for k in OUTPUTS:
        assert math.isfinite(worst[k]) and worst[k] > 0
        assert rec["K"][k] == pow2_at_least(4.0 * rec["ratio"][k]), f"{k}: K is not what the recorded ratio gives"
        assert 4.0 * worst[k] <= rec["K"][k], f"{k}: measured ratio {worst[k]:.4f} is not covered by K = {rec['K'][k]}"




def test_bars_notice_one_dropped_contribution(oracle_mod):
    """what the oracle-based tolerances let through: a backward that drops ONE (pixel, entry) contribution of median weight in the
    longest list, the transmittance replay going on as before, and a forward that does the same.  The affected image pixel and
    the Gaussian's feature, uv and opacity rows leave their bars.  (Its conic row need not: the conic bar follows the moments
    about the tile centre, (|u - cx| + |x|)^2 per pixel, which one pixel next to the splat's centre does not reach; printed.)"""
    import dataclasses
    K = json.load(open(PROFILE))["K"]
    sc = cr.scene(oracle_mod, "opaque_100x60")
    wk = cr.scene_walk(sc)
    feat, g = case_inputs(sc, 3)
    ti = int(np.argmax([t.ids.size for t in wk.tiles]))
    t = wk.tiles[ti]
    w = t.w
    cand = np.argwhere(t.applied)
    i, p = cand[np.argsort(w[t.applied])[len(cand) // 2]]
    applied = t.applied.copy()
    applied[i, p] = False
    broken = dataclasses.replace(wk, tiles=wk.tiles[:ti] + [dataclasses.replace(t, applied=applied)] + wk.tiles[ti + 1:])
    img, cimg = cr.forward(wk, feat, BG)
    grads, comps = cr.backward(wk, sc.conic, sc.opacity, feat, BG, g)
    img_b, _ = cr.forward(broken, feat, BG)
    grads_b, _ = cr.backward(broken, sc.conic, sc.opacity, feat, BG, g, companions=False)
    k = int(t.ids[i])
    print("dropped weight", w[i, p], "of Gaussian", k, "list position", int(i), "of", t.nlist)
    assert cr.worst_ratio(img_b, img, K["image"] * cimg) > 1
    for name in ("feature", "uv", "opacity", "conic"):
        r = cr.worst_ratio(grads_b[name][k], grads[name][k], K[name] * comps[name][k])
        print(name, "error / bar", r)
        assert r > 1 or name == "conic", (name, r)


def record(o):
    """the document of profiles/composite_reference_cpu_float32.json (tools/composite_reference_report.py --backend float32)"""
    worst = measure(o)
    scenes = {}
    for name in SCENES:
        sc = cr.scene(o, name)
        wk = cr.scene_walk(sc)
        scenes[name] = dict(N=int(sc.N), culled=int(sc.culled.size), pruned=int(sc.pruned.size), passes=[int(p) for p in sc.passes],
                            pruned_ids=[int(i) for i in sc.pruned], evaluations=wk.evaluations(), M_max_log2=round(wk.Mmax(), 3))
    return dict(what="numpy float32 restatement of the compositing kernels' arithmetic against tests/composite_ref.py (float64): worst "
                     "|error| / companion per output over the cases; K = smallest power of two >= 4 x ratio",
                backend="numpy_float32", S=cr.S_CLEAR, cases=[dict(scene=n, C=c, K=k, truncation=t) for n, c, k, t in CASES],
                ratio={k: float(f"{v:.4g}") for k, v in worst.items()}, K={k: pow2_at_least(4.0 * float(f"{v:.4g}")) for k, v in worst.items()},
                scenes=scenes)
