"""tests/frames_composite_ref.py on the CPU: the clips of the frame-batch compositing tests are decision-clear, keep the
coverage the GPU tests rely on, and their bars are attainable by float32 arithmetic of the kernels' form with the K values of
profiles/composite_reference_cpu_float32.json unchanged (4 x ratio <= K on every non-empty frame).  The L1 targets put no
element of the fused gradient on a decision.  Sensitivity: one frame's pair records read one slot off in the reduction, or
one contribution dropped in one frame only, leave the bars."""
import dataclasses

import numpy as np
import pytest

import composite_ref as cr
import frames_composite_ref as fr
import gauss_backward_ref as gb
from test_composite_ref_cpu import case_inputs

CLIPS = ("opaque_x4", "hard_x2")
BG = 0.3
K = fr.K_BAR


def frame_inputs(cl, f, C=3):
    return fr.features(cl, C, True)[f], fr.upstream(cl, C)[f]


@pytest.mark.parametrize("name", CLIPS)
def test_every_frame_is_decision_clear(oracle_mod, name):
    cl = fr.clip(oracle_mod, name)
    assert len({sc.name for sc in cl.frames}) == cl.F, "every frame has a name of its own"
    for sc in cl.frames:
        assert sc.N == cl.P and (sc.W, sc.H) == (cl.W, cl.H)
        assert sc.passes[-1] == 0 and not np.isin(sc.pruned, sc.idx).any()
        for Kk, trunc in ((0, False), (20, False), (2, True)):
            assert cr.scene_walk(sc, Kk, trunc).unclear_ids().size == 0, (sc.name, Kk, trunc)


def test_coverage_of_the_clips(oracle_mod):
    cl = fr.clip(oracle_mod, "opaque_x4")
    f0, f1, f2, f3 = cl.frames
    assert cl.opacity_per_frame and not np.array_equal(f2.opacity, f0.opacity)
    assert np.array_equal(f2.opacity, (f0.opacity * np.float32(0.8)).astype(np.float32))
    assert np.array_equal(f2.uv[:, 0], np.float32(cl.W) - f0.uv[:, 0]) and np.array_equal(f2.conic[:, 1], -f0.conic[:, 1])
    assert np.array_equal(f3.depth, (f0.depth.max() + f0.depth.min()) - f0.depth) and np.array_equal(f3.uv, f0.uv)
    # the empty frame in mid-batch: no pairs; its reference is the background, final_T = 1, ncontrib = 0, all-zero gradient rows
    assert np.asarray(f1.idx).size == 0 and not np.asarray(f1.tr).any() and not f1.radius.any()
    feat, g = frame_inputs(cl, 1)
    wk = cr.scene_walk(f1)
    img, _ = cr.forward(wk, feat, BG)
    fT, nc, _ = wk.image_maps()
    assert (img == BG).all() and (fT == 1).all() and (nc == 0).all()
    grads, comps = cr.backward(wk, f1.conic, f1.opacity, feat, BG, g)
    assert all(not grads[k].any() and not comps[k].any() for k in cr.GRADS)
    pairs = [int(np.asarray(sc.idx).size) for sc in cl.frames]
    assert pairs[1] == 0 and len(set(pairs)) == 4, "a different list per frame"
    for sc in (f2, f3):
        cov = cr.coverage(sc, cr.scene_walk(sc))
        print(sc.name, "pruned", sc.pruned.size, sc.passes, "pairs", np.asarray(sc.idx).size, {k: v for k, v in cov.items() if k != "lengths"})
        assert sc.pruned.size <= 0.05 * sc.N
        assert cov["lengths"].max() > 256 and cov["long_to_end"], "lists that run past 256 entries to their end"
        assert cov["quarter_applied_64"] > 60, "more than 60 applied entries of one quarter inside 64 list positions"
        assert cov["stopped_pixels"] > 0
    cov = cr.coverage(f3, cr.scene_walk(f3))
    assert cov["empty"] >= 1 and 17 in cov["saturated_tiles"], "the reversed-depth frame keeps an empty and a saturated tile"
    hard = fr.clip(oracle_mod, "hard_x2")
    h0, h1 = hard.frames
    assert not hard.opacity_per_frame and np.array_equal(h0.opacity, h1.opacity)
    assert not np.array_equal(h0.idx, h1.idx) and np.asarray(h1.idx).size > 0
    ids = fr.NONFINITE_ROWS
    assert any(e - b >= 3 and np.isin(h1.idx[b + 1:e - 1], ids).any() for b, e in h1.tr), "a NaN / inf entry in mid-list"


@pytest.mark.parametrize("name", CLIPS)
def test_float32_restatement_stays_inside_a_quarter_of_the_bars(oracle_mod, name):
    """the condition that lets the GPU tests reuse K on the derived frames: 4 x ratio <= K for every output of every non-empty
    frame, with the inputs K was measured with (test_composite_ref_cpu.case_inputs at C = 3: a property of the frame's geometry.
    The image ratio moves with the feature table: the per-frame tables of the GPU tests give up to 0.60 where this one gives
    0.32 .. 0.44 on the derived frames; K stays what the profile records.)"""
    cl = fr.clip(oracle_mod, name)
    for f, sc in enumerate(cl.frames):
        if np.asarray(sc.idx).size == 0:
            continue
        feat, g = case_inputs(sc, 3)
        wk = cr.scene_walk(sc)
        img, cimg = cr.forward(wk, feat, BG)
        fT, nc, gi = wk.image_maps()
        grads, comps = cr.backward(wk, sc.conic, sc.opacity, feat, BG, g)
        r = cr.f32_forward_backward(sc.uv, sc.conic, sc.opacity, feat, sc.idx, sc.tr, BG, sc.W, sc.H, g)
        assert np.array_equal(r["ncontrib"], nc) and np.array_equal(r["gs_idx"], gi), sc.name
        for a, t in zip(r["applied"], wk.tiles):
            assert np.array_equal(a[:t.ids.size], t.applied) and not a[t.ids.size:].any(), f"{sc.name}: applied structure of tile {t.tile}"
        ratios = dict(image=cr.worst_ratio(r["image"], img, cimg), final_T=cr.worst_ratio(r["final_T"], fT, wk.final_T_companion()))
        finite = np.ones(sc.N, bool)
        if name == "hard_x2":
            finite[fr.NONFINITE_ROWS] = False
        for k in ("uv", "conic", "opacity", "feature", "abs_uv"):
            ratios[k] = cr.worst_ratio(r["grads"][k].reshape(sc.N, -1)[finite], grads[k].reshape(sc.N, -1)[finite],
                                       comps[k].reshape(sc.N, -1)[finite])
        print(sc.name, {k: f"{v:.3g}/{K[k]}" for k, v in ratios.items()})
        for k, v in ratios.items():
            assert 4.0 * v <= K[k], f"{sc.name} {k}: ratio {v:.4f} is not covered by K = {K[k]}"


def test_l1_targets_leave_no_sign_on_a_decision(oracle_mod):
    cl = fr.clip(oracle_mod, "opaque_x4")
    c0, cn, bg = fr.PLANS["3|1|19"]
    feats, _ = fr.sets_inputs(cl, "3|1|19")
    for f, sc in enumerate(cl.frames):
        for g in range(3):
            _, img, cimg = fr.forward_ref(sc, ("sets", "3|1|19", g), feats[g][f], bg[g])
            tgt, s = fr.l1_target(img, cimg, 900 + 10 * f + g)
            bar = K["image"] * cimg
            d = img - tgt.astype(np.float64)
            # every prediction in [img - bar, img + bar] lies on the same side of the float32 target
            assert (np.abs(d) > bar).all() and (np.sign(d) == -s).all()
            assert (np.sign(img - bar - tgt) == -s).all() and (np.sign(img + bar - tgt) == -s).all()
            assert np.abs(d).min() > 0.04


def _clip_check(cl, got_frames, refs):
    """the GPU tests' check over a clip: per frame name -> ratio"""
    return [fr.check_grads_frame(sc, got, *ref) for sc, got, ref in zip(cl.frames, got_frames, refs)]


def test_bars_notice_records_read_one_slot_off(oracle_mod):
    """the pair records of a clip as the tile kernels lay them out ([F, capacity, stride], a record per pair at its slot), from the
    float64 backward of every tile; reduced per frame they are inside the bars -- and outside when ONE frame is read at
    (f * capacity + 1) * stride, the slot of the neighbouring pair"""
    cl = fr.clip(oracle_mod, "opaque_x4")
    lay = gb.plain_layout(3, True)
    cap = max(int(np.asarray(sc.idx).size) for sc in cl.frames) + fr.SLACK
    recs, goffs, refs = [], [], []
    for f, sc in enumerate(cl.frames):
        feat, g = frame_inputs(cl, f)
        rec, goff = fr.host_records(sc, feat, BG, g, lay, cap)
        recs.append(rec)
        goffs.append(goff)
        refs.append(fr.backward_ref(sc, ("cpu", 3), feat, BG, g))
    flat = np.stack(recs).reshape(-1)
    stride = lay["stride"]

    def reduced(shift_frame=None):
        return [fr.slice_record_sums(fr.host_segment_sum(flat, (f * cap + (1 if f == shift_frame else 0)) * stride, stride, goffs[f]), lay)
                for f in range(cl.F)]          # (reads ``flat`` as it is when called)

    ok = _clip_check(cl, reduced(), refs)
    print("in place", ok)
    assert all(v <= 1 for r in ok for v in r.values())
    off = _clip_check(cl, reduced(2), refs)
    print("frame 2 one slot off", off[2])
    assert all(v > 1 for v in off[2].values()), off[2]
    assert off[0] == ok[0] and off[3] == ok[3]
    # not only through the NaN of the first unowned slot: with zeros there every output still leaves its bar
    flat = np.nan_to_num(flat)
    off = _clip_check(cl, reduced(2), refs)
    print("the same, unowned slots zero", off[2])
    assert all(v > 1 for v in off[2].values()), off[2]    # (infinite: a row that must stay zero receives its neighbour's records)


def test_bars_notice_one_contribution_dropped_in_one_frame(oracle_mod):
    """composite_ref's dropped (pixel, entry) contribution of median weight in the longest list, in frame 2 of the clip only: that
    frame's image pixel and the Gaussian's feature, uv and opacity rows leave their bars, the other frames stay exact"""
    cl = fr.clip(oracle_mod, "opaque_x4")
    sc = cl.frames[2]
    wk = cr.scene_walk(sc)
    ti = int(np.argmax([t.ids.size for t in wk.tiles]))
    t = wk.tiles[ti]
    cand = np.argwhere(t.applied)
    i, p = cand[np.argsort(t.w[t.applied])[len(cand) // 2]]
    applied = t.applied.copy()
    applied[i, p] = False
    broken = dataclasses.replace(wk, tiles=wk.tiles[:ti] + [dataclasses.replace(t, applied=applied)] + wk.tiles[ti + 1:])
    k = int(t.ids[i])
    got, refs, imgs = [], [], []
    for f, s in enumerate(cl.frames):
        feat, g = frame_inputs(cl, f)
        ref = fr.backward_ref(s, ("cpu", 3), feat, BG, g)
        refs.append(ref)
        w = broken if f == 2 else cr.scene_walk(s)
        got.append({n: v for n, v in cr.backward(w, s.conic, s.opacity, feat, BG, g, companions=False)[0].items() if n != "bias"})
        _, img, cimg = fr.forward_ref(s, ("cpu", 3), feat, BG)
        imgs.append(fr.ratio(cr.forward(w, feat, BG)[0], img, cimg, K["image"]))
    r = _clip_check(cl, got, refs)
    print("image", imgs, "frame 2", r[2])
    assert imgs[2] > 1 and imgs[0] == imgs[1] == imgs[3] == 0
    assert all(v == 0 for f in (0, 1, 3) for v in r[f].values())
    row = fr.check_grads_frame(sc, {n: np.where(np.arange(sc.N).reshape((-1,) + (1,) * (v.ndim - 1)) == k, v, refs[2][0][n])
                                    for n, v in got[2].items()}, *refs[2])
    for name in ("feature", "uv", "opacity"):
        assert row[name] > 1, (name, row)
