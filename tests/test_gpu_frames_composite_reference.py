"""The frame batch's compositing entry points of csrc/blend.hip against the float64 reference of tests/composite_ref.py, on the
decision-clear clips of tests/frames_composite_ref.py, by the rules of tests/test_gpu_composite_reference.py: ncontrib, gs_idx and
(through them) the applied structure exact on every pixel of every frame; image, final_T and every per-Gaussian gradient row of
every frame within K x companion, K from profiles/composite_reference_cpu_float32.json (nothing here is fitted to a kernel:
tests/test_frames_composite_ref_cpu.py shows that the derived frames keep 4 x float32 ratio <= K).  No budget, no outliers.

What the per-frame file cannot reach and this one does: the frame as a grid dimension (F = 4 with another list per frame, an
empty frame in mid-batch, `capacity` = the fullest frame's pairs + 37 with every unowned slot NaN / -1, opacity and features per
frame and shared, per-frame packed records, cull words and pair-record segments), rows described by feature sources and set
tables, the SMALL instantiations of the one-pass sets backward (a detached set of <= 4 and <= 8 channels), the L1-fused
backward with its tile sums, the chunk entries of a wide set, and the reach-masked lists against an independent walk.

The gradients are the pair records the tile kernels write, reduced per frame with splat_pair_records_segment_sum at
f * capacity * stride and goff_incl[f].  Every case prints its worst ratios; tools/composite_reference_report.py
--backend hip-frames writes them to profiles/frames_composite_reference_gpu.json."""
import dataclasses

import numpy as np
import pytest
import torch

import composite_ref as cr
import frames_composite_ref as fr
import gauss_backward_ref as gb

pytestmark = pytest.mark.gpu

K_BAR = fr.K_BAR
BG = 0.3
FWD_C = [1, 2, 3, 5, 8, 12, 16, 17, 20, 23, 24, 32]
WORST = {}                # route -> output -> worst ratio (err / bar) seen in this process
NONFINITE_WRITES = {}     # route -> frame -> what the kernels wrote into the gradient rows of non-finite operands
_BATCH = {}


def _oracle():
    import oracle
    oracle.build()
    oracle.set_threads(1)
    return oracle


def batch(o, gpu, name, frames=None):
    key = (name, frames)
    if key not in _BATCH:
        cl = fr.clip(o, name)
        _BATCH[key] = fr.Batch(cl if frames is None else cl.sub(frames), gpu)
    return _BATCH[key]


def record(route, ratios):
    w = WORST.setdefault(route, {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), float(v))
    print(route, {k: round(float(v), 4) for k, v in ratios.items()})


def host(t):
    return t.detach().cpu().numpy()


def table_of(per_frame, f):
    return f if per_frame else 0


def check_forward(route, B, fw, feat, key, bg, K=0, trunc=False):
    """every frame of a forward against its float64 walk; feat [F,P,C] (host), key(f) names frame f's feature table"""
    out, fT, nc = host(fw["out"]), host(fw["final_T"]), host(fw["ncontrib"])
    gi = host(fw["gs_idx"]) if K else None
    for f, sc in enumerate(B.clip.frames):
        wk, img, cimg = fr.forward_ref(sc, key(f), feat[f], bg, K, trunc)
        r = fr.check_forward_frame(sc, wk, img, cimg, out[f], fT[f], nc[f], gi[f] if K else None)
        record(route, r)
        assert r["image"] <= 1 and r["final_T"] <= 1, f"{route} frame {f} ({sc.name}) bg={bg} K={K}: {r}"


def check_records(route, B, rec, stride, lay, refs):
    """the per-frame reduction of the pair records against refs[f] = (grads, comps)"""
    assert lay["stride"] == stride
    sums = fr.reduce_frames(B, rec, stride)
    for f, sc in enumerate(B.clip.frames):
        got = fr.slice_record_sums(sums[f], lay)
        got = {k: v for k, v in got.items() if k in refs[f][0]}
        nf = NONFINITE_WRITES.setdefault(route, {}).setdefault(f"frame{f}", {}) if sc.name.startswith("hard") else None
        if np.asarray(sc.idx).size:
            for k in got:
                assert np.abs(np.nan_to_num(refs[f][0][k])).max() > 0, f"{route}: the reference gradient of {k} in frame {f} is all zero"
        r = fr.check_grads_frame(sc, got, *refs[f], nonfinite=nf)
        record(route, r)
        bad = {k: v for k, v in r.items() if not v <= 1}
        assert not bad, f"{route} frame {f} ({sc.name}): outside the bar: {bad} (all: {r})"


# ------------------------------------------------------------------ forward_batch
def run_forward(route, B, C, bg, per_frame, cull, K=0, trunc=False, bgc=None):
    cl = B.clip
    feat = fr.features(cl, C, per_frame)
    d_feat = fr.dev(feat if per_frame else feat[0], B.dev)
    fw = fr.forward_batch(B, C, d_feat, cl.P * C if per_frame else 0, 0.0 if bgc is not None else bg,
                          bgc=None if bgc is None else fr.dev(bgc, B.dev), K=K, trunc=trunc, cull=cull)
    check_forward(route, B, fw, feat, lambda f: ("tab", C, table_of(per_frame, f)), bg if bgc is None else bgc, K, trunc)
    return fw


@pytest.mark.parametrize("C", FWD_C)
def test_forward_batch(gpu, oracle_mod, C):
    Bo, Bh = batch(oracle_mod, gpu, "opaque_x4"), batch(oracle_mod, gpu, "hard_x2")
    run_forward("forward_batch", Bo, C, 0.0, True, True)
    run_forward("forward_batch", Bo, C, 1.0, False, False)
    run_forward("forward_batch_hard", Bh, C, 1.0, False, True)
    run_forward("forward_batch_hard", Bh, C, 0.0, True, False)
    if C in (3, 23):
        bgc = np.random.default_rng(40 + C).uniform(size=C).astype(np.float32)
        run_forward("forward_batch_bg_channels", Bo, C, None, True, True, bgc=bgc)
    if C in (3, 23, 24):
        for B, tag in ((Bo, ""), (Bh, "_hard")):
            run_forward("forward_batch_enhanced" + tag, B, C, BG, True, True, K=20)
            run_forward("forward_batch_truncated" + tag, B, C, BG, True, True, K=2, trunc=True)


@pytest.mark.parametrize("C", [3, 23])
def test_forward_batch_single_frame_gives_the_batch_s_bits(gpu, oracle_mod, C):
    B4, B1 = batch(oracle_mod, gpu, "opaque_x4"), batch(oracle_mod, gpu, "opaque_x4", (0,))
    a = run_forward("forward_batch", B4, C, BG, True, True, K=20)
    b = run_forward("forward_batch_F1", B1, C, BG, True, True, K=20)
    for k in ("out", "final_T", "ncontrib", "gs_idx"):
        assert torch.equal(a[k][0].view(torch.int32), b[k][0].view(torch.int32)), f"{k}: frame 0 of F = 4 differs from the F = 1 run"


# ------------------------------------------------------------------ forward_batch_sources / _sets
def test_forward_batch_sets_and_sources(gpu, oracle_mod):
    B = batch(oracle_mod, gpu, "opaque_x4")
    cl, P = B.clip, B.clip.P
    name = "3|1|19"
    plan = fr.PLANS[name]
    c0, cn, bg = plan
    feats, _ = fr.sets_inputs(cl, name)
    row = fr.sets_row(cl, name, feats)
    bgc = fr.plan_bgc(plan)
    d_bgc = fr.dev(bgc, gpu)
    ref = fr.forward_batch(B, 23, fr.dev(row, gpu), P * 23, 0.0, bgc=d_bgc, K=20)
    tens = [fr.dev(feats[0][0], gpu), fr.dev(feats[1], gpu), fr.dev(feats[2][0], gpu)]      # rgb shared | depth per frame | attributes shared
    a = fr.forward_batch_sets(B, 23, plan, tens, [0, P, 0], d_bgc, K=20)
    b = fr.forward_batch_sources(B, 23, [(c0[g], cn[g], tens[g], [0, P, 0][g]) for g in range(3)], d_bgc, K=20)
    for f, sc in enumerate(cl.frames):
        for g in range(3):
            wk, img, cimg = fr.forward_ref(sc, ("sets", name, g), feats[g][f], bg[g], 20, False)
            r = fr.check_forward_frame(sc, wk, img, cimg, host(a["out"][f, c0[g]:c0[g] + cn[g]]), host(a["final_T"][f]), host(a["ncontrib"][f]),
                                       host(a["gs_idx"][f]))
            record("forward_batch_sets", r)
            assert r["image"] <= 1 and r["final_T"] <= 1, (f, g, r)
    for k in ("out", "final_T", "ncontrib", "gs_idx", "pack"):
        assert torch.equal(a[k].view(torch.int32), ref[k].view(torch.int32)), f"forward_batch_sets {k}: not the bits of forward_batch on the row"
        assert torch.equal(b[k].view(torch.int32), ref[k].view(torch.int32)), f"forward_batch_sources {k}: not the bits of forward_batch on the row"
    # four sources 2 | 1 | 5 | 4, the second and the third per frame
    widths, pf = (2, 1, 5, 4), (False, True, True, False)
    parts = [fr.features(cl, w, p, 7000 + i) for i, (w, p) in enumerate(zip(widths, pf))]
    row = np.ascontiguousarray(np.concatenate(parts, axis=-1))
    bgc = np.random.default_rng(12).uniform(size=12).astype(np.float32)
    d_bgc = fr.dev(bgc, gpu)
    ref = fr.forward_batch(B, 12, fr.dev(row, gpu), P * 12, 0.0, bgc=d_bgc)
    src, c = [], 0
    for w, p, a_ in zip(widths, pf, parts):
        src.append((c, w, fr.dev(a_ if p else a_[0], gpu), P * w if p else 0))
        c += w
    s = fr.forward_batch_sources(B, 12, src, d_bgc)
    check_forward("forward_batch_sources", B, s, row, lambda f: ("src4", f), bgc)
    for k in ("out", "final_T", "ncontrib", "pack"):
        assert torch.equal(s[k].view(torch.int32), ref[k].view(torch.int32)), f"forward_batch_sources {k}: not the bits of forward_batch on the row"


# ------------------------------------------------------------------ backward_batch
def run_backward(route, B, C, want_abs, kind="normal", cull=True):
    cl = B.clip
    feat, g = fr.features(cl, C, True), fr.upstream(cl, C, kind)
    fw = fr.forward_batch(B, C, fr.dev(feat, B.dev), cl.P * C, BG)
    rec, stride = fr.backward_batch(B, C, fw, fr.dev(g, B.dev), BG, want_abs, cull)
    refs = [fr.backward_ref(sc, ("tab", C, f, kind), feat[f], BG, g[f]) for f, sc in enumerate(cl.frames)]
    check_records(route, B, rec, stride, gb.plain_layout(C, want_abs), refs)


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("want_abs", [0, 1])
def test_backward_batch_quarter(gpu, oracle_mod, C, want_abs):
    run_backward("quarter", batch(oracle_mod, gpu, "opaque_x4"), C, want_abs)


@pytest.mark.parametrize("C", [5, 8])
def test_backward_batch_block_matrix(gpu, oracle_mod, C):
    run_backward("mfma", batch(oracle_mod, gpu, "opaque_x4"), C, 1)


@pytest.mark.parametrize("C", [16, 20, 32])
def test_backward_batch_wide_quarter(gpu, oracle_mod, C):
    run_backward("wide_quarter", batch(oracle_mod, gpu, "opaque_x4"), C, 0)


@pytest.mark.parametrize("C", [3, 8])
def test_backward_batch_block_level_without_cull_words(gpu, oracle_mod, C):
    run_backward("block_no_cull", batch(oracle_mod, gpu, "opaque_x4"), C, 1, cull=False)


@pytest.mark.parametrize("route,C,want_abs", [("quarter_single_pixels", 3, 1), ("mfma_single_pixels", 8, 1), ("wide_quarter_single_pixels", 16, 0)])
def test_backward_batch_single_pixels(gpu, oracle_mod, route, C, want_abs):
    run_backward(route, batch(oracle_mod, gpu, "opaque_x4"), C, want_abs, kind="pixel")


@pytest.mark.parametrize("route,C,want_abs", [("quarter_hard", 3, 1), ("mfma_hard", 5, 1), ("wide_quarter_hard", 16, 0)])
def test_backward_batch_hard(gpu, oracle_mod, route, C, want_abs):
    run_backward(route, batch(oracle_mod, gpu, "hard_x2"), C, want_abs)


# ------------------------------------------------------------------ backward_batch_sets / _sets_packed
def sets_case(B, name):
    """inputs of a plan on the device, its forward (forward_batch on the concatenated row) and the per-frame references"""
    cl, P = B.clip, B.clip.P
    plan = fr.PLANS[name]
    c0, cn, bg = plan
    C = sum(cn)
    feats, gims = fr.sets_inputs(cl, name)
    row, grow = fr.sets_row(cl, name, feats), fr.sets_row(cl, name, gims)
    fw = fr.forward_batch(B, C, fr.dev(row, B.dev), P * C, 0.0, bgc=fr.dev(fr.plan_bgc(plan), B.dev))
    own = [None if not cn[g] else fr.dev(feats[g] if g == 1 else feats[g][0], B.dev) for g in range(3)]     # depth per frame, the others shared
    own_dl = [None if not cn[g] else fr.dev(gims[g], B.dev) for g in range(3)]
    refs = [fr.sets_ref(cl, f, name, feats, gims) for f in range(cl.F)]
    return dict(plan=plan, C=C, fw=fw, row=fr.dev(row, B.dev), grow=fr.dev(grow, B.dev), own=own, own_fs=[0, P if cn[1] else 0, 0],
                own_dl=own_dl, refs=refs, feats=feats, gims=gims)


def check_sets(route, B, s, rec, stride, want_abs):
    lay = gb.sets_layout(s["C"])
    refs = s["refs"]
    if not want_abs:     # the abs sums are not formed: their slots hold zeros
        sums = fr.reduce_frames(B, rec, stride)
        assert all(not sums[f][:, list(lay["abs"])].any() for f in range(B.F)), f"{route}: abs slots written without want_abs"
        refs = [({k: v for k, v in g.items() if k != "abs_uv"}, c) for g, c in refs]
    check_records(route, B, rec, stride, lay, refs)


SETS_CASES = [(p, v, a) for p in ("3|1|19", "3|-|10", "3|1|4", "3|1|8", "3|1|9") for v in ("row", "own") for a in (1, 0)]


@pytest.mark.parametrize("name,variant,want_abs", SETS_CASES)
def test_backward_batch_sets(gpu, oracle_mod, name, variant, want_abs):
    """the one-pass backward with the forward's cull words (blend_bwd_sets_quarter_kernel: the renderer's plan staging the
    forward's records, the generic routing, and its SMALL instantiations for a detached set of <= 4 / <= 8 channels), the
    features and image gradients given as the row or as the sets' own tensors"""
    B = batch(oracle_mod, gpu, "opaque_x4")
    s = sets_case(B, name)
    kw = dict(feature=s["row"], feature_fs=B.P * s["C"], dL=s["grow"]) if variant == "row" else \
        dict(set_feature=s["own"], set_fs=s["own_fs"], set_dL=s["own_dl"])
    rec, stride = fr.backward_batch_sets(B, s["C"], s["plan"], s["fw"], want_abs, forward_pack=s["fw"]["pack"], **kw)
    check_sets(f"sets_{name}_{variant}", B, s, rec, stride, want_abs)


@pytest.mark.parametrize("want_abs", [1, 0])
def test_backward_batch_sets_packing_launch_and_block_level(gpu, oracle_mod, want_abs):
    """plan 3|1|19 without the forward's records (the packing launch; both entries) and without the cull words (blend_bwd_sets_kernel)"""
    B = batch(oracle_mod, gpu, "opaque_x4")
    s = sets_case(B, "3|1|19")
    kw = dict(set_feature=s["own"], set_fs=s["own_fs"], set_dL=s["own_dl"])
    rec, stride = fr.backward_batch_sets(B, 23, s["plan"], s["fw"], want_abs, forward_pack=None, **kw)
    check_sets("sets_3|1|19_no_forward_pack", B, s, rec, stride, want_abs)
    rec2, _ = fr.backward_batch_sets(B, 23, s["plan"], s["fw"], want_abs, packed=False, **kw)
    assert torch.equal(rec.view(torch.int32), rec2.view(torch.int32)), "_sets and _sets_packed without forward_pack differ"
    rec, stride = fr.backward_batch_sets(B, 23, s["plan"], s["fw"], want_abs, cull=False, forward_pack=s["fw"]["pack"], **kw)
    check_sets("sets_3|1|19_block", B, s, rec, stride, want_abs)


def test_backward_batch_sets_row_by_sources(gpu, oracle_mod):
    """a row described by sources under plan 3|1|8: `feature` and the set pointers NULL, the packing launch reads the row's
    channels back from the forward's records"""
    B = batch(oracle_mod, gpu, "opaque_x4")
    s = sets_case(B, "3|1|8")
    c0, cn, _ = s["plan"]
    src = [(c0[g], cn[g], s["own"][g], s["own_fs"][g]) for g in range(3)]
    fw = fr.forward_batch_sources(B, 12, src, fr.dev(fr.plan_bgc(s["plan"]), gpu))
    for k in ("out", "final_T", "ncontrib"):
        assert torch.equal(fw[k].view(torch.int32), s["fw"][k].view(torch.int32))
    for want_abs in (1, 0):
        rec, stride = fr.backward_batch_sets(B, 12, s["plan"], fw, want_abs, dL=s["grow"], forward_pack=fw["pack"])
        check_sets("sets_3|1|8_sources", B, s, rec, stride, want_abs)


# ------------------------------------------------------------------ backward_batch_sets_l1
def test_backward_batch_sets_l1(gpu, oracle_mod):
    B = batch(oracle_mod, gpu, "opaque_x4")
    cl, F, T = B.clip, B.F, B.T
    s = sets_case(B, "3|1|19")
    c0, cn, bg = s["plan"]
    scale = [float(v) for v in np.random.default_rng(61).uniform(0.2, 2.0, size=3).astype(np.float32)]
    pred = host(s["fw"]["out"])
    tgts, signs, fwd = [], [], []
    for g in range(3):
        per = [fr.forward_ref(sc, ("sets", "3|1|19", g), s["feats"][g][f], bg[g]) for f, sc in enumerate(cl.frames)]
        tg = [fr.l1_target(img, cimg, 900 + 10 * f + g) for f, (_, img, cimg) in enumerate(per)]
        tgts.append(np.stack([t for t, _ in tg]))
        signs.append(np.stack([sg for _, sg in tg]))
        fwd.append(per)
    # the gradient image the kernel forms, on the host from the GPU's own prediction: its signs are the reference's everywhere
    gims = []
    for g in range(3):
        sg = np.sign(pred[:, c0[g]:c0[g] + cn[g]] - tgts[g])
        assert np.array_equal(sg, -signs[g]), f"set {g}: sign(pred - target) differs from the reference's on {int((sg != -signs[g]).sum())} elements"
        gims.append((np.float32(scale[g]) * sg).astype(np.float32))
    sums = fr.nan(gpu, F, T, 3)
    kw = dict(set_feature=s["own"], set_fs=s["own_fs"], forward_pack=s["fw"]["pack"])
    l1 = dict(pred=s["fw"]["out"], targets=[fr.dev(t, gpu) for t in tgts], scale=scale, sums=sums)
    for want_abs in (1, 0):
        sums.fill_(float("nan"))
        rec, stride = fr.backward_batch_sets(B, 23, s["plan"], s["fw"], want_abs, l1=l1, **kw)
        refs = [fr.sets_ref(cl, f, "3|1|19", s["feats"], gims, key="l1") for f in range(F)]
        check_sets("sets_l1", B, dict(s, refs=refs), rec, stride, want_abs)
        rec2, _ = fr.backward_batch_sets(B, 23, s["plan"], s["fw"], want_abs, set_dL=[fr.dev(g_, gpu) for g_ in gims], **kw)
        assert torch.equal(rec.view(torch.int32), rec2.view(torch.int32)), "the fused backward differs from _sets_packed on the same gradient image"
        # l1_sum[F, tiles, 3]: every entry written, each within sum K companion + (n + 2) 2^-24 sum |ref - target|
        got = host(sums)
        assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} entries of l1_sum were not written"
        gx = (cl.W + 15) // 16
        worst = 0.0
        for f in range(F):
            for g in range(3):
                _, img, cimg = fwd[g][f]
                d = np.abs(img - tgts[g][f].astype(np.float64))
                for t in range(T):
                    sl = (slice(None), slice(16 * (t // gx), 16 * (t // gx) + 16), slice(16 * (t % gx), 16 * (t % gx) + 16))
                    ref, n = d[sl].sum(), d[sl].size
                    bar = K_BAR["image"] * cimg[sl].sum() + (n + 2) * cr.EPS * ref
                    worst = max(worst, abs(float(got[f, t, g]) - ref) / bar)
        record("sets_l1", dict(l1_sum=worst))
        assert worst <= 1, f"l1_sum outside its bar: {worst}"


# ------------------------------------------------------------------ the chunk entries of a wide set
def test_chunk_entries(gpu, oracle_mod):
    """a 40-channel set composited as the chunks [0, 32) and [32, 40): each chunk's forward, its backward from the chunk's packed
    records with and without the cull words, and the entry that packs its own records"""
    B = batch(oracle_mod, gpu, "opaque_x4")
    cl, P, C = B.clip, B.clip.P, 40
    feat, g = fr.features(cl, C, False, 88), fr.upstream(cl, C, "normal", 88)
    d_feat, d_g = fr.dev(feat[0], gpu), fr.dev(g, gpu)
    out = fr.nan(gpu, B.F, C, B.H, B.W)
    for c0, cn in ((0, 32), (32, 8)):
        fw = fr.forward_batch_set(B, C, c0, cn, d_feat, 0, BG, out)
        sub = np.ascontiguousarray(feat[:, :, c0:c0 + cn])
        key = lambda f, c0=c0: ("wide40", c0)
        check_forward(f"chunk_forward_{cn}", B, dict(fw, out=out[:, c0:c0 + cn]), sub, key, BG)
        refs = [fr.backward_ref(sc, ("wide40", c0), sub[f], BG, g[f, c0:c0 + cn]) for f, sc in enumerate(cl.frames)]
        for cull in (True, False):
            rec, stride = fr.backward_batch_set_packed(B, C, c0, cn, fw, d_g, BG, cull)
            check_records(f"chunk_packed_{cn}" + ("" if cull else "_no_cull"), B, rec, stride, gb.plain_layout(cn, 0), refs)
        for want_abs in (0, 1):
            rec, stride = fr.backward_batch_set(B, C, c0, cn, d_feat, 0, fw, d_g, BG, want_abs)
            check_records(f"chunk_set_{cn}", B, rec, stride, gb.plain_layout(cn, want_abs), refs)
    assert torch.isfinite(out).all(), "a channel window of the wide output was not written"


# ------------------------------------------------------------------ reach-masked lists
_REACH = {}


def ordered_image(wk, feat, bg):
    """composite_ref.forward's image summed entry by entry over the entries that apply somewhere: two walks with the same applied
    entries do the same float64 additions in the same order (a matrix product's order depends on the list length)"""
    f = np.asarray(feat, np.float64)
    img = np.zeros((f.shape[1], wk.H, wk.W))
    for t in wk.tiles:
        w, acc = t.w, np.zeros((t.nx * t.ny, f.shape[1]))
        for i in np.nonzero(t.applied.any(1))[0]:
            acc += w[i][:, None] * f[t.ids[i]][None, :]
        acc += t.Tf[:, None] * bg
        img[:, t.y0:t.y0 + t.ny, t.x0:t.x0 + t.nx] = acc.T.reshape(-1, t.ny, t.nx)
    return img


def reach_batch(o, gpu):
    """opaque_x4 binned with the reach masks, its lists read back and checked against the full lists and the full-list walk: per
    tile a subsequence, every dropped entry applied on no pixel, the float64 image of the reach-list walk that of the full lists"""
    if "B" in _REACH:
        return _REACH["B"]
    cl = fr.clip(o, "opaque_x4")
    B = fr.Batch(cl, gpu, reach=True)
    frames, dropped = [], 0
    for f, sc in enumerate(cl.frames):
        idx_r, tr_r = B.frame_lists(f)
        wk = cr.scene_walk(sc)
        for t, ((b0, e0), (b1, e1)) in enumerate(zip(np.asarray(sc.tr).reshape(-1, 2), tr_r)):
            full, kept = np.asarray(sc.idx)[b0:e0], idx_r[b1:e1]
            keep = np.isin(full, kept)
            assert np.array_equal(full[keep], kept), f"frame {f} tile {t}: the reach list is no subsequence of the full list"
            drop = np.nonzero(~keep)[0]
            dropped += drop.size
            tw = wk.tiles[t]
            drop = drop[drop < tw.ids.size]
            assert not tw.applied[drop].any(), f"frame {f} tile {t}: a dropped entry applies to a pixel in the full-list walk"
        sr = dataclasses.replace(sc, name=sc.name + "_reach", idx=idx_r, tr=tr_r)
        feat = fr.features(cl, 3, True)[f]
        wr = cr.scene_walk(sr)
        assert wr.unclear_ids().size == 0
        a, b = ordered_image(wk, feat, BG), ordered_image(wr, feat, BG)
        assert np.array_equal(a, b), f"frame {f}: the float64 image of the reach lists differs (max {np.abs(a - b).max()})"
        assert np.array_equal(a, cr.forward(wk, feat, BG)[0]) or np.allclose(a, cr.forward(wk, feat, BG)[0], rtol=0, atol=1e-13)
        assert np.array_equal(wk.image_maps()[0], wr.image_maps()[0])
        frames.append(sr)
    assert dropped > 0, "the reach masks dropped nothing"
    print("reach: pairs", [int(m) for m in B.pairs], "of", [int(np.asarray(s.idx).size) for s in cl.frames])
    B.clip = fr.Clip("opaque_x4_reach", cl.W, cl.H, cl.P, frames, True)
    _REACH["B"] = B
    return B


def test_reach_lists_forward(gpu, oracle_mod):
    B = reach_batch(oracle_mod, gpu)
    for C in (3, 23):
        run_forward("reach_forward", B, C, BG, True, True, K=20)


@pytest.mark.parametrize("route,C,want_abs", [("reach_quarter", 3, 1), ("reach_wide_quarter", 16, 0)])
def test_reach_lists_backward(gpu, oracle_mod, route, C, want_abs):
    run_backward(route, reach_batch(oracle_mod, gpu), C, want_abs)


def measure():
    """every case of this file outside pytest (tools/composite_reference_report.py --backend hip-frames)"""
    gpu = torch.device("cuda:0")
    o = _oracle()
    for C in FWD_C:
        test_forward_batch(gpu, o, C)
    for C in (3, 23):
        test_forward_batch_single_frame_gives_the_batch_s_bits(gpu, o, C)
    test_forward_batch_sets_and_sources(gpu, o)
    for C in (1, 2, 3):
        for a in (0, 1):
            test_backward_batch_quarter(gpu, o, C, a)
    for C in (5, 8):
        test_backward_batch_block_matrix(gpu, o, C)
    for C in (16, 20, 32):
        test_backward_batch_wide_quarter(gpu, o, C)
    for C in (3, 8):
        test_backward_batch_block_level_without_cull_words(gpu, o, C)
    for route, C, a in [("quarter_single_pixels", 3, 1), ("mfma_single_pixels", 8, 1), ("wide_quarter_single_pixels", 16, 0)]:
        test_backward_batch_single_pixels(gpu, o, route, C, a)
    for route, C, a in [("quarter_hard", 3, 1), ("mfma_hard", 5, 1), ("wide_quarter_hard", 16, 0)]:
        test_backward_batch_hard(gpu, o, route, C, a)
    for name, variant, a in SETS_CASES:
        test_backward_batch_sets(gpu, o, name, variant, a)
    for a in (1, 0):
        test_backward_batch_sets_packing_launch_and_block_level(gpu, o, a)
    test_backward_batch_sets_row_by_sources(gpu, o)
    test_backward_batch_sets_l1(gpu, o)
    test_chunk_entries(gpu, o)
    test_reach_lists_forward(gpu, o)
    for route, C, a in [("reach_quarter", 3, 1), ("reach_wide_quarter", 16, 0)]:
        test_reach_lists_backward(gpu, o, route, C, a)
    return WORST, NONFINITE_WRITES
