"""The frame-batched sparse compositing on the GPU (splat_alpha_blending_points_forward_batch / _backward_batch, csrc/query.hip;
FrameBatch.render_dynamic_sets(points=...)) and the track loss on per-query values (splat_track_loss_grad_points, csrc/loss.hip).

(a) the batch forward is bit-equal to the single-frame operator on every frame's slices of the batch's buffers;
(b) its backward, through the frame batch's pair records, against the dense route (the set rendered as a third image, the
    [Q, 3] gradient scattered into that image's gradient).  Both are float32 routes that each carry the project's gradient
    criterion 2e-3 |ref| + 1e-4 max |ref| against the exact value, so they are compared under twice that bound -- the argument
    of tests/test_gpu_alpha_blending_points_backward.py for the same pair of routes.  Values: atol 1e-5 (1 + S) + rtol 1e-4,
    S = the dense render of |feature| at the pixel;
(c) the per-query loss entry is bit-equal to the image entry;
(d) the deterministic flag refuses the backward.

The clip: 1500 Gaussians at 100 x 60, 40 % of them in one disc (as _opaque_scene of the single-frame test), opacity 0.99 within
8 px of the disc's densest pixel (pixels there stop early), and the Gaussians around the image corner farthest from it below
1/255 (that corner tile's list is empty)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dptr.gs as gs
from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import losses
from splatter_a_video_amd import train_step as TS
from splatter_a_video_amd.dynamics import GAUSSIAN_MAJOR, FrameClock, frame_table, positions_batch_forward
from splatter_a_video_amd.frames import FrameBatch
from splatter_a_video_amd.synth import make_scene
from splatter_a_video_amd.tracks import TrackTargets, frame_weights
from test_gpu_alpha_blending_points import _t
from test_gpu_alpha_blending_points_backward import _coverage
from test_gpu_track_loss import _random_batch

pytestmark = pytest.mark.gpu

N, W, H, T, F = 1500, 100, 60, 20, 3
TIMES1, TIMES2 = [0, 7, 13], [4, 2, 19]
GEOM = ("pos_cubic_node", "rotation", "opacity", "scaling")


@functools.lru_cache(maxsize=None)
def _clip():
    """(clock, parameters, extr, rgb [N,3], track_gs [F,N,3], (hx, hy) the dense spot, (ex, ey) a pixel of the emptied corner tile)"""
    sc = make_scene(N, W, H, F=T, seed=21, clustered=0.4, cluster_area=0.03, blobs=1)
    clock = FrameClock(T)
    p = TS.synthetic_video_params(sc, clock, "cuda", attrs=1, seed=22, cubic_sigma=0.01)
    uv = gs.preprocess_ortho(_t(sc.xyz), _t(sc.scale), _t(sc.rotate), _t(sc.extr), W, H, nearest=0.01)[0].cpu().numpy()
    hist, xe, ye = np.histogram2d(uv[:, 0], uv[:, 1], bins=[W // 4, H // 4], range=[[0, W], [0, H]])
    bx, by = np.unravel_index(np.argmax(hist), hist.shape)
    hx, hy = int(xe[bx] + 2), int(ye[by] + 2)
    op = np.clip(sc.opacity.copy(), 1e-4, 1 - 1e-4)
    near = (uv[:, 0] - hx) ** 2 + (uv[:, 1] - hy) ** 2 < 64
    assert near.sum() >= 50
    op[near] = 0.99
    # the corner tile farthest from the dense spot: every Gaussian within 20 px of it falls below 1/255 (no pair is created)
    cx, cy = (0 if hx > W / 2 else W - 1), (0 if hy > H / 2 else H - 1)
    tx0, ty0 = cx // 16 * 16, cy // 16 * 16
    dx = np.maximum(np.maximum(tx0 - uv[:, 0], uv[:, 0] - (tx0 + 15)), 0)
    dy = np.maximum(np.maximum(ty0 - uv[:, 1], uv[:, 1] - (ty0 + 15)), 0)
    far = (dx < 20) & (dy < 20)
    assert not (far & near).any()
    op[far] = 1e-4
    p["opacity"] = _t(np.log(op / (1 - op))).reshape(p["opacity"].shape)
    rng = np.random.default_rng(5)
    rgb = _t(rng.uniform(size=(N, 3)))
    I = clock.interval_num
    with torch.no_grad():
        track_gs = positions_batch_forward(frame_table(clock, TIMES2, "cuda"), p["position"], p["pos_cubic_node"].reshape(N, -1), I,
                                           GAUSSIAN_MAJOR).clone()
    ex, ey = (1 if cx == 0 else W - 2), (1 if cy == 0 else H - 2)
    return clock, p, _t(sc.extr), rgb, track_gs, (hx, hy), (ex, ey)


def _render(fb, sets, params, points=None, sink=None, K=0):
    clock, p, extr = _clip()[:3]
    return fb.render_dynamic_sets(clock, TIMES1, extr, sets, position=p["position"], pos_cubic_node=params["pos_cubic_node"],
                                  rotation=params["rotation"], rot_poly_feat=p["rot_poly_feat"],
                                  rot_fourier_feat=p["rot_fourier_feat"], opacity=params["opacity"], scaling=params["scaling"],
                                  cubic_layout=GAUSSIAN_MAJOR, K=K, grad_sink=sink, points=points)


def _leaves():
    p = _clip()[1]
    out = {k: p[k].detach().clone().requires_grad_(True) for k in GEOM}
    out["pos_cubic_node"] = p["pos_cubic_node"].detach().reshape(N, -1).clone().requires_grad_(True)
    return out


def _offsets(counts):
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------------------------- (a) forward
def _mixed_queries():
    """per-frame query counts (47, 0, 5): integer pixels (a window on the dense spot, the emptied corner tile), points on eighths,
    the image corners, points outside and non-finite points"""
    (hx, hy), (ex, ey) = _clip()[5:]
    nan, inf = float("nan"), float("inf")
    f0 = [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]                                              # the image corners
    f0 += [[x, y] for y in range(hy - 2, hy + 3) for x in range(hx - 2, hx + 3)]                       # 25 integer pixels, dense
    f0 += [[ex, ey], [3, 5], [17, H - 2]]                                                              # integer: empty tile, others
    f0 += [[15.5, 15.5], [15.875, 15.125], [31.5, 15.5], [hx + 0.5, hy + 0.25], [hx - 0.875, hy + 0.5], [ex + 0.25, ey - 0.5],
           [W - 1.5, H - 1.5]]                                                                         # on eighths
    f0 += [[-0.5, 3], [W - 0.125, -0.875], [-5, -5], [1e9, 2]]                                         # partly / fully outside
    f0 += [[nan, 3], [nan, nan], [inf, 2], [2, -inf]]                                                  # not finite
    f2 = [[hx, hy], [40, 30], [20.375, 41.625], [W + 2.5, H + 1], [3, nan]]
    assert len(f0) == 47 and len(f2) == 5
    return np.asarray(f0 + f2, np.float32), [47, 0, 5]


def _forward_batch(fb, op, feat, fs, bg, pts, off, nF=F, frame0=0):
    Q, C = pts.shape[0], feat.shape[-1]
    out = torch.full((Q, C), 7.0, device="cuda")
    cT = torch.full((Q, 4), 7.0, device="cuda")
    cn = torch.full((Q, 4), 7, dtype=torch.int32, device="cuda")
    i64 = ctypes.c_int64
    L.check(L.lib().splat_alpha_blending_points_forward_batch(
        nF, N, C, L.ptr(fb.uv[frame0:]), L.ptr(fb.conic[frame0:]), L.ptr(op), i64(0), L.ptr(feat), i64(fs),
        L.ptr(fb.idx_sorted[frame0:]), L.ptr(fb.tile_range[frame0:]), i64(fb.capacity), bg, W, H, i64(Q), L.ptr(off),
        L.ptr(pts), L.ptr(out), L.ptr(cT), L.ptr(cn), L.stream()))
    return out, cT, cn


@pytest.mark.parametrize("C,per_frame,bg", [(3, True, 0.0), (70, False, 0.75)])
def test_batch_forward_is_the_single_frame_operator_on_every_frame(C, per_frame, bg):
    clock, p, extr, rgb, track_gs, _, _ = _clip()
    fb = FrameBatch(F, N, W, H, 4, "cuda")
    with torch.no_grad():
        _render(fb, [dict(feature=rgb, bg=0.2, taps=True), dict(feature="depth", bg=1.0)], p | {"pos_cubic_node": p["pos_cubic_node"].reshape(N, -1)})
    op = torch.sigmoid(p["opacity"]).reshape(N, 1).contiguous()
    feat = track_gs if per_frame else _t(np.random.default_rng(C).uniform(-1, 1, size=(N, C)))
    pts_np, counts = _mixed_queries()
    pts, off = _t(pts_np), _offsets(counts)
    out, cT, cn = _forward_batch(fb, op, feat, N * C if per_frame else 0, bg, pts, off)
    o = np.concatenate([[0], np.cumsum(counts)])
    early = deep = empty = at64 = 0
    for f in range(F):
        sl = slice(o[f], o[f + 1])
        if o[f] == o[f + 1]:
            continue
        ff = feat[f] if per_frame else feat
        ref, rT, rn = gs.alpha_blending_points(fb.uv[f], fb.conic[f], op, ff, fb.idx_sorted[f], fb.tile_range[f], bg, W, H, pts[sl],
                                               return_corners=True, differentiable=True)
        # the batch entry is the walk of splat_alpha_blending_points_forward_live: a corner without bilinear weight is not walked
        # and reports 0 in both maps, where the operator's return_corners forward walks it -- every other element, bit for bit
        with np.errstate(invalid="ignore"):
            fx, fy = pts_np[sl, 0] - np.floor(pts_np[sl, 0]), pts_np[sl, 1] - np.floor(pts_np[sl, 1])
            wgt = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], 1)
        live = torch.from_numpy(np.nan_to_num(wgt, nan=0.0) != 0).cuda()
        assert torch.equal(out[sl], ref), f
        assert torch.equal(cT[sl], torch.where(live, rT, torch.zeros_like(rT))), f
        assert torch.equal(cn[sl], torch.where(live, rn, torch.zeros_like(rn))), f
        assert int((~live & (rn > 0)).sum()) >= 1 and int((live & (rn > 0)).sum()) >= 1
        geom = (None, None, None, None, fb.tile_range[f], N, W, H)
        e, d, m = _coverage(geom, pts_np[sl], cn[sl])
        early, deep, empty = early + e, deep + d, empty + m
        at64 += int((cn[sl] == 64).sum())
    print(f"corners early-stopped {early}, last >= 65 {deep}, last == 64 {at64}, on an empty list {empty}")
    assert early >= 1 and deep >= 1 and empty >= 1
    if at64 == 0:
        print("this scene gives no corner whose last applied entry is exactly the 64th (the block boundary itself)")
    # a query no frame owns (malformed offsets) writes zeros; the owned ones are unchanged
    bad = off.clone()
    bad[1] = 40                     # queries 40 .. 46 are owned by frame 1 now
    bad[3] = 50                     # queries 50, 51 by nobody
    out2, cT2, cn2 = _forward_batch(fb, op, feat, N * C if per_frame else 0, bg, pts, bad)
    assert torch.equal(out2[:40], out[:40]) and torch.equal(out2[47:50], out[47:50])
    assert float(out2[50:].abs().max()) == 0 and float(cT2[50:].abs().max()) == 0 and int(cn2[50:].abs().max()) == 0
    # F = 1 with a single query (frame 2 of the batch as a batch of its own); Q = 0
    one = _forward_batch(fb, op, feat[2:] if per_frame else feat, N * C if per_frame else 0, bg, pts[47:48], _offsets([1]), nF=1,
                         frame0=2)
    assert torch.equal(one[0], out[47:48]) and torch.equal(one[1], cT[47:48]) and torch.equal(one[2], cn[47:48])
    assert _forward_batch(fb, op, feat, 0, bg, pts[:0], _offsets([0, 0, 0]))[0].shape == (0, C)


# ------------------------------------------------------------------------------------------------------------- (b) backward
def _integer_queries(seed):
    """unique integer query pixels per frame (69-ish, 0, 30-ish): random ones, the image corners, a window on the dense spot"""
    (hx, hy), (ex, ey) = _clip()[5:]
    rng = np.random.default_rng(seed)
    win = {y * W + x for y in range(hy - 2, hy + 3) for x in range(hx - 2, hx + 3)}
    per = [set(rng.choice(W * H, 40, replace=False).tolist()) | {0, W - 1, (H - 1) * W, H * W - 1, ey * W + ex} | win, set(),
           set(rng.choice(W * H, 25, replace=False).tolist()) | {y * W + x for y in range(hy - 1, hy + 2) for x in range(hx, hx + 2)}]
    pix = [np.array(sorted(s), np.int64) for s in per]
    return pix, [len(s) for s in pix]


def _grads_of(leaves, sink, fb):
    return {**{k: leaves[k].grad for k in GEOM}, "track_gs": sink, "tap": fb.tap.clone()}


def _assert_doubled(got, ref, what):
    for k in ref:
        a, b = got[k].double().cpu().numpy().reshape(-1), ref[k].double().cpu().numpy().reshape(-1)
        assert np.isfinite(a).all() and np.abs(b).max() > 0, (what, k)            # every reference gradient is non-zero
        lim = 2.0 * (2e-3 * np.abs(b) + 1e-4 * np.abs(b).max())
        err = np.abs(a - b)
        print(f"{what}: d{k} max |ref| {np.abs(b).max():.3e}, worst err / bound {float((err / lim).max()):.4f}")
        assert (err <= lim).all(), f"{what}: d{k}: {int((err > lim).sum())} of {a.size} off, worst {float((err / lim).max()):.2f} x the bound"


@pytest.mark.parametrize("branch", ["plain", "sources"])
def test_batch_backward_through_the_pair_records_matches_the_dense_route(branch):
    clock, p, extr, rgb, track_gs, _, _ = _clip()
    pix, counts = _integer_queries(seed=3)
    Q = sum(counts)
    allpix = np.concatenate(pix)
    pts = _t(np.stack([allpix % W, allpix // W], 1))
    off = _offsets(counts)
    rng = np.random.default_rng(9)
    g_rgb, g_dep, g_pts = _t(rng.normal(size=(F, 3, H, W))), _t(rng.normal(size=(F, 1, H, W))), _t(rng.normal(size=(Q, 3)))
    # "sources": the rgb set as a list of two tensors -- the row is then described by feature sources (the other Gaussian-side entry)
    rgb_set = (lambda r: [r[:, :2].contiguous(), r[:, 2:].contiguous()]) if branch == "sources" else (lambda r: r)
    fidx = 2 if branch == "sources" else 1

    # ---- route 2 (dense): the set as a third image, its gradient the [Q, 3] gradient scattered to the query pixels
    fb7 = FrameBatch(F, N, W, H, 7, "cuda")
    lv = _leaves()
    sink_d = torch.zeros_like(track_gs)
    sets = [dict(feature=rgb_set(rgb), bg=0.2, taps=True), dict(feature="depth", bg=1.0),
            dict(feature=[track_gs], bg=0.0, detach_opacity=True)]
    o_rgb, o_dep, o_trk, ids = _render(fb7, sets, lv, sink={f"feature:{fidx}": sink_d}, K=8)
    g_img = torch.zeros(F, 3, H * W, device="cuda")
    fr = np.repeat(np.arange(F), counts)
    g_img[torch.from_numpy(fr).cuda(), :, torch.from_numpy(allpix).cuda()] = g_pts
    dense_vals = o_trk.detach().reshape(F, 3, H * W)[torch.from_numpy(fr).cuda(), :, torch.from_numpy(allpix).cuda()]
    torch.autograd.backward([o_rgb, o_dep, o_trk], [g_rgb, g_dep, g_img.view(F, 3, H, W)])
    ref = _grads_of(lv, sink_d, fb7)
    # the atomic accumulation is exercised: a Gaussian among the first contributors of two or more queries of one frame
    idn = ids.cpu().numpy().reshape(F, H * W, -1)
    shared = 0
    for f in range(F):
        hit = idn[f, pix[f]]
        flat = np.concatenate([np.unique(r[r >= 0]) for r in hit]) if len(hit) else np.zeros(0, np.int64)
        shared += int((np.unique(flat, return_counts=True)[1] >= 2).sum()) if flat.size else 0
    assert shared >= 1
    with torch.no_grad():
        S = _render(fb7, [sets[0], sets[1], dict(feature=[track_gs.abs()], bg=0.0, detach_opacity=True)], lv)[2]
        S = S.reshape(F, 3, H * W)[torch.from_numpy(fr).cuda(), :, torch.from_numpy(allpix).cuda()]

    # ---- route 1 (sparse): rgb + depth in the row, the set at its query pixels
    fb4 = FrameBatch(F, N, W, H, 4, "cuda")
    lv = _leaves()
    sink_s = torch.zeros_like(track_gs)
    points = dict(feature=track_gs, points=pts, offsets=off, bg=0.0, detach_opacity=True)
    o_rgb, o_dep, vals, _ = _render(fb4, sets[:2], lv, points=points, sink={"points": sink_s}, K=8)
    assert vals.shape == (Q, 3) and vals.requires_grad
    tol = 1e-5 * (1 + S.double()) + 1e-4 * dense_vals.double().abs()
    err = (vals.detach().double() - dense_vals.double()).abs()
    print(f"values max err / tol {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
    torch.autograd.backward([o_rgb, o_dep, vals], [g_rgb, g_dep, g_pts])
    got = _grads_of(lv, sink_s, fb4)
    _assert_doubled(got, ref, f"sparse vs dense ({branch})")

    # ---- without a sink the feature's gradient comes back through autograd, the same bits up to the atomics' order
    lv2 = _leaves()
    tg = track_gs.clone().requires_grad_(True)
    o = _render(fb4, sets[:2], lv2, points=dict(points, feature=tg))
    torch.autograd.backward(list(o[:3]), [g_rgb, g_dep, g_pts])
    _assert_doubled({"track_gs": tg.grad}, {"track_gs": ref["track_gs"]}, "feature gradient through autograd")

    # ---- a None gradient of the sparse output launches nothing: every gradient is that of the call without points
    lv_a, lv_b = _leaves(), _leaves()
    sink_n = torch.zeros_like(track_gs)
    o = _render(fb4, sets[:2], lv_a, points=points, sink={"points": sink_n})
    torch.autograd.backward(list(o[:2]), [g_rgb, g_dep])
    tap_a = fb4.tap.clone()
    o = _render(fb4, sets[:2], lv_b)
    assert len(o) == 3
    torch.autograd.backward(list(o[:2]), [g_rgb, g_dep])
    for k in GEOM:
        assert torch.equal(lv_a[k].grad, lv_b[k].grad), k
    assert torch.equal(tap_a, fb4.tap) and float(sink_n.abs().max()) == 0


# ------------------------------------------------------------------------------------------------------------- (c) the loss
def test_loss_on_query_values_is_bit_equal_to_the_loss_on_the_image():
    Hh, Ww, Ff = 60, 107, 3
    img, pairs = _random_batch(Ff, Hh, Ww, 3, seed=31, hidden={1})               # frame 1: no visible query
    _, single = _random_batch(Ff, Hh, Ww, 3, seed=31, Q1=True)
    pairs[2] = single[2]                                                          # frame 2: a single query
    tt = TrackTargets.cat([TrackTargets.from_reference(q, t, Hh, Ww) for q, t in pairs])
    pix = tt.pixels.clone()
    pix[5] = pix[4]                 # a duplicate
    pix[9] = Hh * Ww + 3            # out of range (and the next one is then "not above the previous")
    pix[12] = -1
    tt = TrackTargets(tt.offsets, pix, tt.targets, Hh, Ww, tt.counts).to("cuda")
    assert tt.counts[2] == 1 and tt.counts[0] > 100
    Q = tt.Q
    dimg = img.cuda()
    fr = torch.from_numpy(np.repeat(np.arange(Ff), tt.counts)).cuda()
    valid = (tt.pixels >= 0) & (tt.pixels < Hh * Ww)
    safe = torch.where(valid, tt.pixels, torch.zeros_like(tt.pixels)).long()
    values = dimg.reshape(Ff, 3, Hh * Ww)[fr, :, safe].contiguous()
    values[~valid] = 123.0          # never read: the pixel decides that the query is malformed
    w = frame_weights([0, 1, 2], [5, 0, 1], 6).cuda()

    def outs():
        return (torch.full((Ff,), 7.0, device="cuda"), torch.zeros(1, device="cuda"), torch.full((Ff, 2), 7, dtype=torch.int32, device="cuda"))
    g_img = torch.empty_like(dimg)
    per_a, slot_a, cnt_a = outs()
    losses.track_loss_grad(dimg, tt, w, 0.98, 2.0, g_img, per_frame=per_a, loss_slot=slot_a, counts=cnt_a)
    g_val = torch.full((Q, 3), 7.0, device="cuda")
    per_b, slot_b, cnt_b = outs()
    losses.track_loss_points_grad(values, tt, w, 0.98, 2.0, g_val, per_frame=per_b, loss_slot=slot_b, counts=cnt_b)
    assert torch.equal(per_a, per_b) and torch.equal(slot_a, slot_b) and torch.equal(cnt_a, cnt_b)
    assert float(per_a[1]) == 0 and int(cnt_a[1, 0]) == 0 and int(cnt_a[2, 0]) == 1 and float(per_a[0]) > 0
    # a skipped (malformed) query has a zero row; every other row is the image gradient at its pixel
    prev = torch.cat([torch.full((1,), -1, device="cuda", dtype=torch.int32), tt.pixels[:-1]])
    first = torch.zeros(Q, dtype=torch.bool, device="cuda")
    first[tt.offsets[:-1][torch.tensor(tt.counts, device="cuda") > 0]] = True
    skipped = ~valid | (~first & (prev >= tt.pixels))
    assert int(skipped.sum()) >= 4
    at_pix = g_img.reshape(Ff, 3, Hh * Ww)[fr, :, safe]
    assert torch.equal(g_val[~skipped], at_pix[~skipped]) and float(g_val[skipped].abs().max()) == 0
    assert float(g_val[:, 2].abs().max()) == 0 and float(g_val.abs().max()) > 0
    assert int((g_val[:, :2] != 0).sum()) == int((g_img != 0).sum())       # nothing else in the image either
    # no gradient wanted: the same losses
    per_c, slot_c, cnt_c = outs()
    losses.track_loss_points_grad(values, tt, w, 0.98, 2.0, None, per_frame=per_c, loss_slot=slot_c, counts=cnt_c)
    assert torch.equal(per_c, per_a) and torch.equal(cnt_c, cnt_a)


# ------------------------------------------------------------------------------------------------------------- (d) deterministic
def test_deterministic_mode_refuses_the_batch_backward():
    clock, p, extr, rgb, track_gs, _, _ = _clip()
    pix, counts = _integer_queries(seed=4)
    allpix = np.concatenate(pix)
    points = dict(feature=track_gs, points=_t(np.stack([allpix % W, allpix // W], 1)), offsets=_offsets(counts), bg=0.0,
                  detach_opacity=True)
    sets = [dict(feature=rgb, bg=0.2, taps=True), dict(feature="depth", bg=1.0)]
    fb = FrameBatch(F, N, W, H, 4, "cuda")
    lv = {k: v.detach() for k, v in _leaves().items()}
    sink = {k: torch.zeros_like(lv[k]) for k in GEOM}
    sink["points"] = torch.zeros_like(track_gs)
    g = [torch.ones(F, 3, H, W, device="cuda"), torch.ones(F, 1, H, W, device="cuda"), torch.ones(sum(counts), 3, device="cuda")]
    r = rgb.clone().requires_grad_(True)
    o = _render(fb, [dict(sets[0], feature=r), sets[1]], lv, points=points, sink=sink)
    L.set_deterministic(True)
    try:
        with pytest.raises(L.SplatError, match="deterministic"):
            torch.autograd.backward(list(o[:3]), g)
    finally:
        L.set_deterministic(False)
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0 for t in sink.values()) and r.grad is None
    o = _render(fb, [dict(sets[0], feature=r), sets[1]], lv, points=points, sink=sink)
    torch.autograd.backward(list(o[:3]), g)                      # the flag is off again: the backward runs
    assert all(float(t.abs().max()) > 0 for t in sink.values()) and float(r.grad.abs().max()) > 0
