"""The compositing kernels of csrc/blend.hip against the float64 reference of tests/composite_ref.py on decision-clear scenes.

No budget and no undecided mask: on a pruned scene (composite_ref.prune) float32 and float64 make every decision alike, so
ncontrib, gs_idx and (through them) the applied structure are compared exactly on every pixel, and the image, final_T and every
gradient element must lie within K x companion.  The K values are those profiles/composite_reference_cpu_float32.json records
from the numpy float32 restatement (tests/test_composite_ref_cpu.py); nothing here is fitted to the kernels.  A ratio above 1
is a finding about a kernel or about a term the companion lacks.

Scenes (composite_ref.scene): opaque_100x60 (partial tiles in both directions, an empty tile, lists longer than 256 entries
walked to their end, pixels that stop early, a tile that saturates entirely, quarters with 18 applied entries inside one
staged batch; the same with an opacity bias) and hard_64x48 (opacity 0 and 1e-30, needles above 1e4, splats on pixel and tile
centres, NaN / inf rows in mid-list: those rows apply nowhere, their own gradient rows are not compared but recorded, and they
must leave every finite row within its bar).  tests/test_composite_ref_cpu.py asserts the coverage on the CPU.

Routes, each through the public operators (csrc/blend.hip launch_bwd_ab picks the kernel):
  forward         alpha_blending, _enhanced (K = 20; K = 2 with truncation), _with_bias; every chunk width, bg 0 and 1
  quarter         pair lists, C <= 3, |ndc| taps given            mfma     pair lists, C = 5, 8; C = 3 with "bwd_quarters" = 0
  wide_quarter    pair lists, C = 16, 20, 32, no |ndc| taps      pair     deterministic mode (C = 5) and the bias operator
  atomic          the same lists cloned: no pair map is found     sets     alpha_blending_shared: 3 | 1 | 19 and 3 | - | 10,
  chunk2          C = 33: the second chunk accumulates                     "sets_std" 1 and 0; block-level with "bwd_quarters" = 0
The upstream gradient is a seeded normal image; one case per kernel family puts it on a single pixel per tile, so that a
mis-routed pixel cannot average out.  Every case prints its worst ratios; tools/composite_reference_report.py --backend hip
writes them to profiles/composite_reference_gpu.json."""
import json

import numpy as np
import pytest
import torch

import composite_ref as cr
from test_composite_ref_cpu import BG, PROFILE, case_inputs
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

K_BAR = json.load(open(PROFILE))["K"]
FWD_C = [1, 2, 3, 5, 8, 12, 16, 17, 20, 23, 24, 32, 33, 65]
NONFINITE_ROWS = np.arange(150, 166)      # hard_64x48: NaN / inf conic or uv
WORST = {}                                # route -> output -> worst ratio (err / bar) seen in this process
NONFINITE_WRITES = {}                     # route -> what the kernels wrote into the gradient rows of non-finite operands
_LISTS = {}


def _oracle():
    import oracle
    oracle.build()
    oracle.set_threads(1)
    return oracle


def lists(sc, gpu):
    """this library's sort of the scene (carries the pair map): bit-equal to the lists the float64 walk used"""
    import dptr.gs as gs
    if sc.name not in _LISTS:
        idx, tr = gs.sort_gaussian(dev(sc.sort_uv, gpu), dev(sc.depth, gpu), sc.W, sc.H, dev(sc.radius, gpu), dev(sc.tiles, gpu))
        assert np.array_equal(idx.cpu().numpy().reshape(-1), np.asarray(sc.idx).reshape(-1)), "sorted ids differ from the walk's"
        assert np.array_equal(tr.cpu().numpy().reshape(-1, 2), np.asarray(sc.tr).reshape(-1, 2)), "tile ranges differ from the walk's"
        _LISTS[sc.name] = (idx, tr)
    return _LISTS[sc.name]


def record(route, ratios):
    w = WORST.setdefault(route, {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), float(v))
    print(route, {k: round(float(v), 4) for k, v in ratios.items()})


def ratio(got, ref, comp, K, scale=None):
    """worst |got - ref| / (K comp) over the elements; ``scale``: per-column factor applied to ref and bar (the ndc taps), whose
    multiplication rounds once more"""
    ref, comp = np.asarray(ref, np.float64), np.asarray(comp, np.float64)
    bar = K * comp
    if scale is not None:
        ref, bar = ref * scale, bar * scale + 2 * cr.EPS * np.abs(ref * scale)
    return cr.worst_ratio(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, ref, bar)


_FWD_REF = {}


def forward_ref(sc, C, bg, K, trunc):
    key = (sc.name, C, bg, K, trunc)
    if key not in _FWD_REF:
        wk = cr.scene_walk(sc, K, trunc)
        assert wk.unclear_ids().size == 0
        feat, _ = case_inputs(sc, C)
        _FWD_REF[key] = (wk,) + cr.forward(wk, feat, bg)
    return _FWD_REF[key]


def check_forward(route, sc, gpu, C, bg, K=0, trunc=False):
    """one forward launch against the float64 walk; returns (out, leaves) for a backward to follow"""
    import dptr.gs as gs
    idx, tr = lists(sc, gpu)
    wk, img, cimg = forward_ref(sc, C, bg, K, trunc)
    feat, _ = case_inputs(sc, C)
    t = {k: dev(v, gpu).requires_grad_(True) for k, v in dict(uv=sc.uv, conic=sc.conic, opacity=sc.opacity, feature=feat).items()}
    args = (t["uv"], t["conic"], t["opacity"], t["feature"])
    gi = None
    if sc.bias is not None:
        t["bias"] = dev(sc.bias, gpu).requires_grad_(True)
        out = gs.alpha_blending_with_bias(*args, t["bias"], idx, tr, bg, sc.W, sc.H)
    elif K:
        out, nc_out, gi = gs.alpha_blending_enhanced(*args, idx, tr, bg, sc.W, sc.H, K=K, enable_truncation=trunc)
    else:
        out = gs.alpha_blending(*args, idx, tr, bg, sc.W, sc.H)
    saved = out.grad_fn.saved_tensors
    final_T, ncontrib = saved[6], saved[7]
    fT, nc, gi_ref = wk.image_maps()
    assert np.array_equal(ncontrib.cpu().numpy(), nc), f"{route}: ncontrib differs on {int((ncontrib.cpu().numpy() != nc).sum())} pixels"
    if K:
        assert torch.equal(nc_out, ncontrib)
        assert np.array_equal(gi.cpu().numpy(), gi_ref), f"{route}: gs_idx differs on {int((gi.cpu().numpy() != gi_ref).any(-1).sum())} pixels"
    r = dict(image=ratio(out, img, cimg, K_BAR["image"]), final_T=ratio(final_T, fT, wk.final_T_companion(), K_BAR["final_T"]))
    record(route, r)
    assert r["image"] <= 1 and r["final_T"] <= 1, f"{route} C={C} bg={bg} K={K}: {r}"
    return out, t


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("C", FWD_C)
def test_forward_opaque(gpu, oracle_mod, C):
    sc = cr.scene(oracle_mod, "opaque_100x60")
    for bg in (0.0, 1.0):
        check_forward("forward", sc, gpu, C, bg)
    check_forward("forward_enhanced", sc, gpu, C, BG, K=20)
    check_forward("forward_truncated", sc, gpu, C, BG, K=2, trunc=True)
    check_forward("forward_bias", cr.scene(oracle_mod, "opaque_100x60_bias"), gpu, C, BG)


@pytest.mark.parametrize("C", [1, 3, 5, 16, 33])
def test_forward_hard(gpu, oracle_mod, C):
    sc = cr.scene(oracle_mod, "hard_64x48")
    for bg in (0.0, 1.0):
        check_forward("forward_hard", sc, gpu, C, bg)
    check_forward("forward_hard_enhanced", sc, gpu, C, BG, K=20)
    check_forward("forward_hard_truncated", sc, gpu, C, BG, K=2, trunc=True)


# ------------------------------------------------------------------ backward
def upstream(sc, C, kind):
    _, g = case_inputs(sc, C)
    if kind == "pixel":     # one pixel per tile, another place in every tile
        m = np.zeros((sc.H, sc.W), bool)
        gx, gy = (sc.W + 15) // 16, (sc.H + 15) // 16
        for t in range(gx * gy):
            x0, y0 = 16 * (t % gx), 16 * (t // gx)
            nx, ny = min(16, sc.W - x0), min(16, sc.H - y0)
            m[y0 + (5 * t + 3) % ny, x0 + (7 * t + 1) % nx] = True
        g = g * m[None]
    return g


_BWD_REF = {}


def backward_ref(sc, C, bg, kind, feat=None, g=None, key=None):
    key = key or (sc.name, C, bg, kind)
    if key not in _BWD_REF:
        wk = cr.scene_walk(sc)
        if feat is None:
            feat, g = case_inputs(sc, C)[0], upstream(sc, C, kind)
        _BWD_REF[key] = cr.backward(wk, sc.conic, sc.opacity, feat, bg, g)
    return _BWD_REF[key]


def compare_grads(route, sc, got, grads, comps):
    """got: name -> tensor (uv, conic, opacity, feature, bias, ndc, abs_ndc); every finite row within K x companion"""
    half = np.array([[0.5 * sc.W, 0.5 * sc.H]])
    finite = np.ones(sc.N, bool)
    if sc.name.startswith("hard"):
        finite[NONFINITE_ROWS] = False
        w = NONFINITE_WRITES.setdefault(route, {})
        for name, tns in got.items():
            rows = tns.detach().cpu().numpy().reshape(sc.N, -1)[NONFINITE_ROWS]
            w[name] = dict(nan=int(np.isnan(rows).sum()), inf=int(np.isinf(rows).sum()), nonzero=int((np.nan_to_num(rows) != 0).sum()),
                           elements=int(rows.size))
    r = {}
    for name, tns in got.items():
        src = dict(ndc="uv", abs_ndc="abs_uv").get(name, name)
        a = tns.detach().cpu().numpy().reshape(sc.N, -1)[finite]
        ref = grads[src].reshape(sc.N, -1)[finite]
        cmp_ = comps[src].reshape(sc.N, -1)[finite]
        assert np.abs(ref).max() > 0, f"{route}: the reference gradient of {name} is all zero"
        r[name] = ratio(a, ref, cmp_, K_BAR[src], half if name in ("ndc", "abs_ndc") else None)
    record(route, r)
    bad = {k: v for k, v in r.items() if not v <= 1}
    assert not bad, f"{route}: outside the bar: {bad} (all: {r})"


def run_backward(route, sc, gpu, C, kind="normal", taps=True, clone_lists=False, K=0):
    import dptr.gs as gs
    idx, tr = lists(sc, gpu)
    if clone_lists:
        idx, tr = idx.clone(), tr.clone()
    feat, _ = case_inputs(sc, C)
    g = upstream(sc, C, kind)
    t = {k: dev(v, gpu).requires_grad_(True) for k, v in dict(uv=sc.uv, conic=sc.conic, opacity=sc.opacity, feature=feat).items()}
    if taps:
        t["ndc"] = torch.zeros(sc.N, 2, device=gpu, requires_grad=True)
        t["abs_ndc"] = torch.zeros(sc.N, 2, device=gpu, requires_grad=True)
    tap = (t["ndc"], t["abs_ndc"]) if taps else ()
    args = (t["uv"], t["conic"], t["opacity"], t["feature"])
    if sc.bias is not None:
        t["bias"] = dev(sc.bias, gpu).requires_grad_(True)
        out = gs.alpha_blending_with_bias(*args, t["bias"], idx, tr, BG, sc.W, sc.H, *tap)
    elif K:
        out = gs.alpha_blending_enhanced(*args, idx, tr, BG, sc.W, sc.H, *tap, K=K)[0]
    else:
        out = gs.alpha_blending(*args, idx, tr, BG, sc.W, sc.H, *tap)
    out.backward(dev(g, gpu))
    torch.cuda.synchronize()
    grads, comps = backward_ref(sc, C, BG, kind)
    compare_grads(route, sc, {k: v.grad for k, v in t.items()}, grads, comps)


@pytest.mark.parametrize("C", [1, 2, 3])
def test_backward_quarter(gpu, oracle_mod, C):
    run_backward("quarter", cr.scene(oracle_mod, "opaque_100x60"), gpu, C)


def test_backward_quarter_enhanced_and_single_pixels(gpu, oracle_mod):
    sc = cr.scene(oracle_mod, "opaque_100x60")
    run_backward("quarter", sc, gpu, 3, K=20)
    run_backward("quarter_single_pixels", sc, gpu, 3, kind="pixel")


@pytest.mark.parametrize("C", [5, 8])
def test_backward_block_matrix(gpu, oracle_mod, C):
    run_backward("mfma", cr.scene(oracle_mod, "opaque_100x60"), gpu, C)


def test_backward_block_matrix_narrow_and_single_pixels(gpu, oracle_mod):
    from splatter_a_video_amd import _lib as L
    sc = cr.scene(oracle_mod, "opaque_100x60")
    old = L.get_option("bwd_quarters")
    L.set_option("bwd_quarters", 0)
    try:
        run_backward("mfma", sc, gpu, 3)
    finally:
        L.set_option("bwd_quarters", old)
    run_backward("mfma_single_pixels", sc, gpu, 8, kind="pixel")


@pytest.mark.parametrize("C", [16, 20, 32])
def test_backward_wide_quarter(gpu, oracle_mod, C):
    run_backward("wide_quarter", cr.scene(oracle_mod, "opaque_100x60"), gpu, C, taps=False)


def test_backward_wide_quarter_single_pixels(gpu, oracle_mod):
    run_backward("wide_quarter_single_pixels", cr.scene(oracle_mod, "opaque_100x60"), gpu, 16, kind="pixel", taps=False)


def test_backward_pair_kernel_deterministic_and_bias(gpu, oracle_mod):
    from splatter_a_video_amd import _lib as L
    was = L.deterministic()
    L.set_deterministic(True)
    try:
        run_backward("pair", cr.scene(oracle_mod, "opaque_100x60"), gpu, 5)
    finally:
        L.set_deterministic(was)
    run_backward("pair_bias", cr.scene(oracle_mod, "opaque_100x60_bias"), gpu, 3)


@pytest.mark.parametrize("C", [3, 5])
def test_backward_atomic(gpu, oracle_mod, C):
    run_backward("atomic", cr.scene(oracle_mod, "opaque_100x60"), gpu, C, clone_lists=True)


def test_backward_atomic_bias(gpu, oracle_mod):
    run_backward("atomic_bias", cr.scene(oracle_mod, "opaque_100x60_bias"), gpu, 3, clone_lists=True)


def test_backward_second_chunk(gpu, oracle_mod):
    run_backward("chunk2", cr.scene(oracle_mod, "opaque_100x60"), gpu, 33)


@pytest.mark.parametrize("route,C,kw", [("quarter_hard", 3, {}), ("mfma_hard", 5, {}), ("wide_quarter_hard", 16, dict(taps=False)),
                                        ("atomic_hard", 3, dict(clone_lists=True))])
def test_backward_hard(gpu, oracle_mod, route, C, kw):
    run_backward(route, cr.scene(oracle_mod, "hard_64x48"), gpu, C, **kw)


# ------------------------------------------------------------------ several sets, one backward pass
PLANS = {"3|1|19": ((3, 1, 19), (0.25, 1.0, 0.0), (False, False, True), (True, False, False)),
         "3|-|10": ((3, 10), (0.25, 0.0), (False, True), (True, False))}


SETS_CASES = [("3|1|19", 1, 1), ("3|1|19", 0, 1), ("3|-|10", 1, 1), ("3|-|10", 0, 1), ("3|1|19", 1, 0)]   # plan, sets_std, bwd_quarters


@pytest.mark.parametrize("plan,std,quarters", SETS_CASES)
def test_backward_sets(gpu, oracle_mod, plan, std, quarters):
    """blend_bwd_sets_quarter_kernel (the renderer's plan staging the forward's records, or the generic slot -> channel routing)
    and, with "bwd_quarters" = 0, the block-level blend_bwd_sets_kernel"""
    import dptr.gs as gs
    from splatter_a_video_amd import _lib as L
    sc = cr.scene(oracle_mod, "opaque_100x60")
    widths, bgs, detach, taps = PLANS[plan]
    idx, tr = lists(sc, gpu)
    rng = np.random.default_rng(2000 + sum(widths))
    feats = [rng.uniform(-1, 1, size=(sc.N, w)).astype(np.float32) for w in widths]
    gims = [rng.normal(size=(w, sc.H, sc.W)).astype(np.float32) for w in widths]
    t = {k: dev(v, gpu).requires_grad_(True) for k, v in dict(uv=sc.uv, conic=sc.conic, opacity=sc.opacity).items()}
    tf = [dev(f, gpu).requires_grad_(True) for f in feats]
    ndc = torch.zeros(sc.N, 2, device=gpu, requires_grad=True)
    andc = torch.zeros(sc.N, 2, device=gpu, requires_grad=True)
    old = L.get_option("sets_std"), L.get_option("bwd_quarters")
    L.set_option("sets_std", std)
    L.set_option("bwd_quarters", quarters)
    try:
        res = gs.alpha_blending_shared(t["uv"], t["conic"], t["opacity"], tf, idx, tr, list(bgs), sc.W, sc.H, ndc, andc, K=20,
                                       detach_opacity=list(detach), taps=list(taps))
        imgs, nc, gi = res[:len(widths)], res[len(widths)], res[len(widths) + 1]
        sum((im * dev(g, gpu)).sum() for im, g in zip(imgs, gims)).backward()
        torch.cuda.synchronize()
    finally:
        L.set_option("sets_std", old[0])
        L.set_option("bwd_quarters", old[1])
    route = f"sets_{plan}_std{std}" + ("" if quarters else "_block")
    wk = cr.scene_walk(sc, 20, False)
    fT, nc_ref, gi_ref = wk.image_maps()
    assert np.array_equal(nc.cpu().numpy(), nc_ref) and np.array_equal(gi.cpu().numpy(), gi_ref)
    tot = {k: 0.0 for k in ("uv", "conic", "opacity", "abs_uv", "tap_uv")}
    ctot = dict(tot)
    fwd, got = {}, dict(uv=t["uv"].grad, conic=t["conic"].grad, opacity=t["opacity"].grad, ndc=ndc.grad, abs_ndc=andc.grad)
    for s, (f, g, bg) in enumerate(zip(feats, gims, bgs)):
        img, cimg = cr.forward(wk, f, bg)
        fwd[f"image{s}"] = ratio(imgs[s], img, cimg, K_BAR["image"])
        gr, cp = backward_ref(sc, widths[s], bg, "sets", f, g, key=(sc.name, plan, s))
        for k in ("uv", "conic"):
            tot[k], ctot[k] = tot[k] + gr[k], ctot[k] + cp[k]
        if not detach[s]:
            tot["opacity"], ctot["opacity"] = tot["opacity"] + gr["opacity"], ctot["opacity"] + cp["opacity"]
        if taps[s]:
            tot["abs_uv"], ctot["abs_uv"] = tot["abs_uv"] + gr["abs_uv"], ctot["abs_uv"] + cp["abs_uv"]
            tot["tap_uv"], ctot["tap_uv"] = tot["tap_uv"] + gr["uv"], ctot["tap_uv"] + cp["uv"]
        r = ratio(tf[s].grad, gr["feature"], cp["feature"], K_BAR["feature"])
        fwd[f"feature{s}"] = r
    record(route, fwd)
    assert all(v <= 1 for v in fwd.values()), f"{route}: {fwd}"
    half = np.array([[0.5 * sc.W, 0.5 * sc.H]])
    r = dict(uv=ratio(got["uv"], tot["uv"], ctot["uv"], K_BAR["uv"]), conic=ratio(got["conic"], tot["conic"], ctot["conic"], K_BAR["conic"]),
             opacity=ratio(got["opacity"].reshape(-1), tot["opacity"], ctot["opacity"], K_BAR["opacity"]),
             ndc=ratio(got["ndc"], tot["tap_uv"], ctot["tap_uv"], K_BAR["uv"], half),
             abs_ndc=ratio(got["abs_ndc"], tot["abs_uv"], ctot["abs_uv"], K_BAR["abs_uv"], half))
    record(route, r)
    assert all(v <= 1 for v in r.values()), f"{route}: {r}"


def measure():
    """every case of this file outside pytest (tools/composite_reference_report.py): route -> output -> worst ratio"""
    gpu = torch.device("cuda:0")
    o = _oracle()
    for C in FWD_C:
        test_forward_opaque(gpu, o, C)
    for C in (1, 3, 5, 16, 33):
        test_forward_hard(gpu, o, C)
    for C in (1, 2, 3):
        test_backward_quarter(gpu, o, C)
    test_backward_quarter_enhanced_and_single_pixels(gpu, o)
    for C in (5, 8):
        test_backward_block_matrix(gpu, o, C)
    test_backward_block_matrix_narrow_and_single_pixels(gpu, o)
    for C in (16, 20, 32):
        test_backward_wide_quarter(gpu, o, C)
    test_backward_wide_quarter_single_pixels(gpu, o)
    test_backward_pair_kernel_deterministic_and_bias(gpu, o)
    for C in (3, 5):
        test_backward_atomic(gpu, o, C)
    test_backward_atomic_bias(gpu, o)
    test_backward_second_chunk(gpu, o)
    for route, C, kw in [("quarter_hard", 3, {}), ("mfma_hard", 5, {}), ("wide_quarter_hard", 16, dict(taps=False)),
                         ("atomic_hard", 3, dict(clone_lists=True))]:
        test_backward_hard(gpu, o, route, C, kw)
    for plan, std, quarters in SETS_CASES:
        test_backward_sets(gpu, o, plan, std, quarters)
    return WORST, NONFINITE_WRITES
