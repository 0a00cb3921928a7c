"""The sparse compositing kernels of csrc/query.hip against the float64 reference of tests/points_ref.py on decision-clear scenes
and clips, by the rules of tests/test_gpu_composite_reference.py: corner_ncontrib exact; out, corner_T and every gradient element
within K x companion, element-wise, no outlier budget.  K per output is what profiles/points_reference_cpu_float32.json resolves
from the numpy float32 restatement (tests/test_points_ref_cpu.py): the dense K where 4 x ratio <= K, else a sparse K of its own.
Nothing here is fitted to a kernel; a ratio above 1 is a finding about a kernel or about a term the companion lacks.

Entry points (include/splat_hip.h, "point tracking"):
  _forward, _forward_live          through the C ABI with NaN / -1 prefilled outputs: every C of both the accumulator boundary (64,
                                   65) and the launch boundary (256, 257), bg 0 and 0.75, both scenes
  _backward, _backward_ordered     through dptr.gs.alpha_blending_points(differentiable=True[, ordered=True]) on this library's own
                                   sort (bit-equal to the walk's lists; it carries the pair map): a normal upstream and one that is
                                   non-zero on one query per tile only, a detached opacity, repeated queries, integer pixels (one live
                                   corner per query), a tile with more than 64 live corners; BOTH against the float64 reference
  _forward_batch, _backward_batch, _backward_batch_ordered   through the C ABI on the clips of tests/frames_composite_ref.py
                                   (opaque_x4: an empty frame, a mirrored frame, a reversed depth order; hard_x2), queries in CSR
                                   form with another set per frame, feature stride 0 and per frame, detach_opacity 0 and 1, a frame
                                   without queries.  The tile backward of the same forward runs first with an upstream image of
                                   its own: the geometry gradients, reduced per frame as frames_composite_ref.reduce_frames does it,
                                   are compared with dense + sparse reference under the sum of the two bars; with a zero dense
                                   upstream the sparse contribution stands alone.
On the hard scene and clip the gradient rows of the NaN / inf Gaussians are recorded, not compared; every finite row must stay
within its bar.  Every case prints its worst ratios; tools/composite_reference_report.py --backend hip-points writes them to
profiles/points_composite_reference_gpu.json."""
import numpy as np
import pytest
import torch

import composite_ref as cr
import frames_composite_ref as fr
import gauss_backward_ref as gb
import points_ref as pr
from test_gpu_composite_reference import lists
from test_gpu_parity import dev
from test_points_ref_cpu import NONFINITE_ROWS, finite_rows, reference

pytestmark = pytest.mark.gpu

K_BAR = pr.k_bar()
K_DENSE = pr.dense_k()
BG = 0.3
FWD_C = [1, 3, 19, 64, 65, 256, 257, 300]
BWD_C = [1, 3, 19, 70, 257]
WORST = {}                # route -> output -> worst ratio (err / bar) seen in this process
NONFINITE_WRITES = {}     # route -> what the kernels wrote into the gradient rows of non-finite operands
_BATCH = {}


def _oracle():
    import oracle
    oracle.build()
    oracle.set_threads(1)
    return oracle


def _L():
    import splatter_a_video_amd._lib as L
    return L


def record(route, ratios):
    w = WORST.setdefault(route, {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), float(v))
    print(route, {k: round(float(v), 4) for k, v in ratios.items()})


def host(t):
    return t.detach().cpu().numpy()


def check_forward_values(route, what, fw, out, corner_T, corner_n):
    """out [Q,C], corner_T [Q,4], corner_n [Q,4] (host) against a points_ref.forward result"""
    assert np.array_equal(corner_n, fw["corner_n"]), f"{route} {what}: corner_ncontrib differs on {int((corner_n != fw['corner_n']).sum())} corners"
    r = dict(out=cr.worst_ratio(out, fw["out"], K_BAR["out"] * pr.out_companion(fw, K_DENSE["image"])),
             corner_T=cr.worst_ratio(corner_T, fw["corner_T"], K_BAR["corner_T"] * fw["corner_T_comp"]))
    record(route, r)
    assert r["out"] <= 1 and r["corner_T"] <= 1, f"{route} {what}: {r}"


# ------------------------------------------------------------------ _forward and _forward_live
def run_forward(sc, gpu, C, bg):
    L = _L()
    idx, tr = lists(sc, gpu)
    ref = reference(sc, C, bg, backward=False)
    Q = len(ref["pts"])
    t = [dev(a, gpu) for a in (sc.uv, sc.conic, sc.opacity, ref["feat"])]
    pts = dev(ref["pts"], gpu)
    for live in (False, True):
        out, cT, cn = fr.nan(gpu, Q, C), fr.nan(gpu, Q, 4), fr.minus(gpu, Q, 4)
        fn = L.lib().splat_alpha_blending_points_forward_live if live else L.lib().splat_alpha_blending_points_forward
        L.check(fn(sc.N, C, L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(idx), L.ptr(tr), float(bg), sc.W, sc.H, Q,
                   L.ptr(pts), L.ptr(out), L.ptr(cT), L.ptr(cn), L.stream()))
        torch.cuda.synchronize()
        route = ("forward_live" if live else "forward") + ("_hard" if sc.name.startswith("hard") else "")
        check_forward_values(route, f"C={C} bg={bg}", ref["live" if live else "fwd"], host(out), host(cT), host(cn))


@pytest.mark.parametrize("C", FWD_C)
def test_forward_and_forward_live(gpu, oracle_mod, C):
    for name in ("opaque_100x60", "hard_64x48"):
        for bg in (0.0, 0.75):
            run_forward(cr.scene(oracle_mod, name), gpu, C, bg)


def test_forward_through_the_operator(gpu, oracle_mod):
    import dptr.gs as gs
    sc = cr.scene(oracle_mod, "opaque_100x60")
    idx, tr = lists(sc, gpu)
    ref = reference(sc, 3, BG, backward=False)
    t = [dev(a, gpu) for a in (sc.uv, sc.conic, sc.opacity, ref["feat"])]
    out, cT, cn = gs.alpha_blending_points(*t, idx, tr, BG, sc.W, sc.H, dev(ref["pts"], gpu), return_corners=True)
    check_forward_values("forward", "operator", ref["fwd"], host(out), host(cT), host(cn))


# ------------------------------------------------------------------ _backward and _backward_ordered
def compare_grads(route, sc, got, grads, comps, K=None):
    """got: name -> [N, k] host array; every finite row within its bar (K x companion, or the bars given as comps with K = 1)"""
    fin = finite_rows(sc)
    if not fin.all():
        w = NONFINITE_WRITES.setdefault(route, {})
        for name, a in got.items():
            rows = np.asarray(a).reshape(sc.N, -1)[NONFINITE_ROWS]
            w[name] = dict(nan=int(np.isnan(rows).sum()), inf=int(np.isinf(rows).sum()), nonzero=int((np.nan_to_num(rows) != 0).sum()),
                           elements=int(rows.size))
    r = {}
    for name, a in got.items():
        k = 1.0 if K is None else K[name]
        r[name] = cr.worst_ratio(np.asarray(a).reshape(sc.N, -1)[fin], grads[name].reshape(sc.N, -1)[fin],
                                 k * comps[name].reshape(sc.N, -1)[fin])
    record(route, r)
    bad = {k: v for k, v in r.items() if not v <= 1}
    assert not bad, f"{route} ({sc.name}): outside the bar: {bad} (all: {r})"


def run_backward(route, sc, gpu, C, ordered, kind="normal", detach=False):
    import dptr.gs as gs
    idx, tr = lists(sc, gpu)
    ref = reference(sc, C, BG, kind)
    t = {k: dev(v, gpu).requires_grad_(True) for k, v in dict(uv=sc.uv, conic=sc.conic, opacity=sc.opacity, feature=ref["feat"]).items()}
    if detach:
        t["opacity"] = t["opacity"].detach()
    out = gs.alpha_blending_points(t["uv"], t["conic"], t["opacity"], t["feature"], idx, tr, BG, sc.W, sc.H, dev(ref["pts"], gpu),
                                   differentiable=True, ordered=ordered)
    corner_T, corner_n = out.grad_fn.saved_tensors[-2:]
    check_forward_values(route, f"C={C} {kind}: its forward", ref["live"], host(out), host(corner_T), host(corner_n))
    out.backward(dev(ref["g"], gpu))
    torch.cuda.synchronize()
    assert not detach or t["opacity"].grad is None
    got = {k: host(v.grad) for k, v in t.items() if v.grad is not None}
    assert set(got) == set(pr.GRADS) - ({"opacity"} if detach else set())
    for k in got:
        assert np.abs(ref["grads"][k]).max() > 0, f"{route}: the reference gradient of {k} is all zero"
    compare_grads(route, sc, got, ref["grads"], ref["comps"], K_BAR)


ROUTES = [("atomic", False), ("ordered", True)]


@pytest.mark.parametrize("C", BWD_C)
@pytest.mark.parametrize("route,ordered", ROUTES)
def test_backward(gpu, oracle_mod, route, ordered, C):
    run_backward(route, cr.scene(oracle_mod, "opaque_100x60"), gpu, C, ordered)


@pytest.mark.parametrize("route,ordered", ROUTES)
def test_backward_one_query_per_tile(gpu, oracle_mod, route, ordered):
    sc = cr.scene(oracle_mod, "opaque_100x60")
    run_backward(route + "_one_per_tile", sc, gpu, 3, ordered, kind="one_per_tile")
    run_backward(route + "_one_per_tile", sc, gpu, 70, ordered, kind="one_per_tile")


@pytest.mark.parametrize("route,ordered", ROUTES)
def test_backward_detached_opacity_repeated_queries_and_integer_pixels(gpu, oracle_mod, route, ordered):
    sc = cr.scene(oracle_mod, "opaque_100x60")
    run_backward(route + "_detached", sc, gpu, 3, ordered, detach=True)
    run_backward(route + "_repeated", sc, gpu, 3, ordered, kind="repeat")
    run_backward(route + "_integer", sc, gpu, 3, ordered, kind="integer")


@pytest.mark.parametrize("route,ordered", ROUTES)
def test_backward_hard(gpu, oracle_mod, route, ordered):
    sc = cr.scene(oracle_mod, "hard_64x48")
    run_backward(route + "_hard", sc, gpu, 3, ordered)
    run_backward(route + "_hard_one_per_tile", sc, gpu, 19, ordered, kind="one_per_tile")


# ------------------------------------------------------------------ the frame batch
def batch(o, gpu, name):
    if name not in _BATCH:
        _BATCH[name] = fr.Batch(fr.clip(o, name), gpu)
    return _BATCH[name]


def batch_case(cl, C, per_frame, no_queries=None):
    """per frame the reference of its own query set (seed = frame, another feature table per frame or one for all), the CSR arrays"""
    refs = [reference(sc, C, BG, "integer" if f == no_queries else "normal", seed=f, table=f if per_frame else 0)
            for f, sc in enumerate(cl.frames)]
    counts = [0 if f == no_queries else len(r["pts"]) for f, r in enumerate(refs)]
    keep = [f for f in range(cl.F) if f != no_queries]
    pts = np.concatenate([refs[f]["pts"] for f in keep])
    g = np.concatenate([refs[f]["g"] for f in keep])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    feat = np.stack([r["feat"] for r in refs]) if per_frame else refs[0]["feat"]
    return refs, counts, pts, g, offsets, feat


def points_forward_batch(B, C, feat, feat_fs, pts, offsets):
    L = _L()
    Q = int(pts.shape[0])
    o = dict(out=fr.nan(B.dev, Q, C), corner_T=fr.nan(B.dev, Q, 4), corner_n=fr.minus(B.dev, Q, 4))
    L.check(L.lib().splat_alpha_blending_points_forward_batch(
        B.F, B.P, C, L.ptr(B.uv), L.ptr(B.conic), L.ptr(B.opacity), B.op_fs, L.ptr(feat), feat_fs, L.ptr(B.idx_sorted),
        L.ptr(B.tile_range), B.cap, BG, B.W, B.H, Q, L.ptr(offsets), L.ptr(pts), L.ptr(o["out"]), L.ptr(o["corner_T"]),
        L.ptr(o["corner_n"]), L.stream()))
    torch.cuda.synchronize()
    return o


def points_backward_batch(B, C, feat, feat_fs, pts, offsets, fw, g, rec, stride, detach, dfeat, dfeat_fs, ordered):
    L = _L()
    lib = L.lib()
    Q = int(pts.shape[0])
    head = (B.F, B.P, C, L.ptr(B.uv), L.ptr(B.conic), L.ptr(B.opacity), B.op_fs, L.ptr(feat), feat_fs, L.ptr(B.idx_sorted),
            L.ptr(B.tile_range), B.cap, BG, B.W, B.H, Q, L.ptr(offsets), L.ptr(pts), L.ptr(fw["corner_T"]), L.ptr(fw["corner_n"]),
            L.ptr(g), L.ptr(B.slot_sorted), L.ptr(rec), stride, int(detach), L.ptr(dfeat), dfeat_fs)
    if ordered:
        need = int(lib.splat_alpha_blending_points_backward_batch_ordered_scratch_bytes(B.F, C, B.W, B.H, Q, B.cap))
        assert need > 0
        scratch = fr.nan(B.dev, (need + 3) // 4)
        L.check(lib.splat_alpha_blending_points_backward_batch_ordered(*head, L.ptr(B.goff), L.ptr(scratch), scratch.numel() * 4, L.stream()))
    else:
        L.check(lib.splat_alpha_blending_points_backward_batch(*head, L.stream()))
    torch.cuda.synchronize()


DENSE_C = 3


def run_batch(route, B, C, ordered, per_frame, detach, dense_upstream=True, no_queries=None):
    cl = B.clip
    refs, counts, pts_h, g_h, off_h, feat_h = batch_case(cl, C, per_frame, no_queries)
    # ---- the dense row of the same batch: its forward, then its tile backward writes every pair record
    dfeat_h = fr.features(cl, DENSE_C, True)
    dg_h = fr.upstream(cl, DENSE_C) if dense_upstream else np.zeros((cl.F, DENSE_C, cl.H, cl.W), np.float32)
    dfw = fr.forward_batch(B, DENSE_C, fr.dev(dfeat_h, B.dev), cl.P * DENSE_C, BG)
    rec, stride = fr.backward_batch(B, DENSE_C, dfw, fr.dev(dg_h, B.dev), BG, 0)
    lay = gb.plain_layout(DENSE_C, 0)
    assert lay["stride"] == stride
    # ---- the sparse set on the same lists
    feat, feat_fs = fr.dev(feat_h, B.dev), (cl.P * C if per_frame else 0)
    pts, off, g = fr.dev(pts_h, B.dev), fr.dev(off_h, B.dev), fr.dev(g_h, B.dev)
    fw = points_forward_batch(B, C, feat, feat_fs, pts, off)
    out, cT, cn = (pr.split(off_h, host(fw[k])) for k in ("out", "corner_T", "corner_n"))
    for f in range(cl.F):
        if f != no_queries:
            check_forward_values(route + "_forward", f"frame {f}", refs[f]["live"], out[f], cT[f], cn[f])
    dfeat = torch.zeros((cl.F, cl.P, C) if per_frame else (cl.P, C), dtype=torch.float32, device=B.dev)
    points_backward_batch(B, C, feat, feat_fs, pts, off, fw, g, rec, stride, detach, dfeat, cl.P * C if per_frame else 0, ordered)
    # ---- geometry: the records reduced per frame = dense + sparse, under the sum of the two bars
    sums = fr.reduce_frames(B, rec, stride)
    live = [f for f in range(cl.F) if f != no_queries]
    for f, sc in enumerate(cl.frames):
        got = fr.slice_record_sums(sums[f], lay)
        dgr, dcp = fr.backward_ref(sc, ("pts_dense", DENSE_C, f), dfeat_h[f], BG, dg_h[f]) if (np.asarray(sc.idx).size and dense_upstream) \
            else fr.zero_refs(sc.N, DENSE_C)
        tot, bar = {}, {}
        for k in ("uv", "conic", "opacity"):
            sparse = f in live and not (k == "opacity" and detach)
            tot[k] = dgr[k] + (refs[f]["grads"][k] if sparse else 0.0)
            bar[k] = K_DENSE[k] * dcp[k] + (K_BAR[k] * refs[f]["comps"][k] if sparse else 0.0)
        tot["feature"], bar["feature"] = dgr["feature"], K_DENSE["feature"] * dcp["feature"]      # the dense row's: untouched
        compare_grads(f"{route}_frame{f}" if sc.name.startswith("hard") else route, sc, {k: got[k] for k in tot}, tot, bar)
    # ---- the sparse feature gradient: per frame, or summed over the frames
    d = host(dfeat)
    if per_frame:
        for f in range(cl.F):
            if f in live:
                compare_grads(route, cl.frames[f], dict(sparse_feature=d[f]), dict(sparse_feature=refs[f]["grads"]["feature"]),
                              dict(sparse_feature=K_BAR["feature"] * refs[f]["comps"]["feature"]))
            else:
                assert not d[f].any(), f"{route}: frame {f} has no queries and a feature gradient"
    else:
        compare_grads(route, cl.frames[0], dict(sparse_feature=d), dict(sparse_feature=sum(refs[f]["grads"]["feature"] for f in live)),
                      dict(sparse_feature=K_BAR["feature"] * sum(refs[f]["comps"]["feature"] for f in live)))
    assert any(np.abs(refs[f]["grads"]["uv"]).max() > 0 for f in live)


BATCH_CASES = [(3, True, 0, True, None), (3, False, 1, True, None), (3, True, 0, False, None), (3, False, 0, True, 2), (70, True, 1, True, None)]


@pytest.mark.parametrize("C,per_frame,detach,dense_upstream,no_queries", BATCH_CASES)
@pytest.mark.parametrize("route,ordered", ROUTES)
def test_batch(gpu, oracle_mod, route, ordered, C, per_frame, detach, dense_upstream, no_queries):
    run_batch("batch_" + route + ("" if dense_upstream else "_alone"), batch(oracle_mod, gpu, "opaque_x4"), C, ordered, per_frame, detach,
              dense_upstream, no_queries)


@pytest.mark.parametrize("route,ordered", ROUTES)
def test_batch_hard(gpu, oracle_mod, route, ordered):
    run_batch("batch_" + route + "_hard", batch(oracle_mod, gpu, "hard_x2"), 3, ordered, True, 0)


def measure():
    """every case of this file outside pytest (tools/composite_reference_report.py): route -> output -> worst ratio"""
    gpu = torch.device("cuda:0")
    o = _oracle()
    for C in FWD_C:
        test_forward_and_forward_live(gpu, o, C)
    test_forward_through_the_operator(gpu, o)
    for route, ordered in ROUTES:
        for C in BWD_C:
            test_backward(gpu, o, route, ordered, C)
        test_backward_one_query_per_tile(gpu, o, route, ordered)
        test_backward_detached_opacity_repeated_queries_and_integer_pixels(gpu, o, route, ordered)
        test_backward_hard(gpu, o, route, ordered)
        for case in BATCH_CASES:
            test_batch(gpu, o, route, ordered, *case)
        test_batch_hard(gpu, o, route, ordered)
    return WORST, NONFINITE_WRITES
