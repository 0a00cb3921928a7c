"""FrameBatch.render_dynamic_sets(points=dict(..., ordered=True)) (splat_alpha_blending_points_backward_batch_ordered,
csrc/query.hip) on the clip of tests/test_gpu_points_batch.py.

Values: the ordered route against the unordered (float-atomic) route of the same call under that module's bound (`_assert_doubled`,
2 x (2e-3 |ref| + 1e-4 max |ref|)): the two compute the same sums in another order.
Bits: the ordered route's own sums are isolated by ZERO image gradients (the tile backward then writes zero records whichever
kernel it takes, so every non-zero bit of every gradient comes from the ordered adds): three runs and a run under the deterministic
flag are bit-equal.  With real image gradients the whole backward is compared under the flag, where every kernel of the library is
free of float atomics.
Unchanged: what the ordered route does not add to (the taps, the image sets' feature gradient; with a None gradient of the sparse
output everything) has the bits of a call without the sparse set's gradient."""
import numpy as np
import pytest
import torch

from splatter_a_video_amd import _lib as L
from splatter_a_video_amd.frames import FrameBatch
from test_gpu_alpha_blending_points import _t
from test_gpu_points_batch import F, GEOM, H, N, W, _assert_doubled, _clip, _integer_queries, _leaves, _mixed_queries, _offsets, _render

pytestmark = pytest.mark.gpu

SHARE = [k for k in GEOM if k != "opacity"] + ["track_gs"]      # what the sparse set's gradient reaches (its opacity is detached)


def _queries(kind):
    if kind == "integer":
        pix, counts = _integer_queries(seed=3)
        allpix = np.concatenate(pix)
        return _t(np.stack([allpix % W, allpix // W], 1)), counts
    pts, counts = _mixed_queries()
    return _t(pts), counts


def _image_grads(zero=False):
    rng = np.random.default_rng(9)
    g_rgb, g_dep = _t(rng.normal(size=(F, 3, H, W))), _t(rng.normal(size=(F, 1, H, W)))
    return (torch.zeros_like(g_rgb), torch.zeros_like(g_dep)) if zero else (g_rgb, g_dep)


def _run(fb, ordered, feature, pts, off, g_pts, g_img, how="sink", points_grad=True):
    """one forward + backward; returns the gradients of the geometry leaves, of the sparse feature, of the rgb feature, the taps.
    how = "sink": geometry and sparse feature through grad_sink; "autograd": both come back through autograd."""
    clock, p, extr, rgb, track_gs, _, _ = _clip()
    lv = _leaves()
    r = rgb.clone().requires_grad_(True)
    sets = [dict(feature=r, bg=0.2, taps=True), dict(feature="depth", bg=1.0)]
    feat = feature.clone()
    sink = None
    if how == "sink":       # the geometry gradients and the sparse feature's gradient are ADDED to the caller's buffers
        lv = {k: v.detach() for k, v in lv.items()}
        sink = {k: torch.zeros_like(lv[k]) for k in GEOM}
        sink["points"] = torch.zeros_like(feat)
    else:
        feat.requires_grad_(True)
    points = dict(feature=feat, points=pts, offsets=off, bg=0.0, detach_opacity=True, ordered=ordered)
    o = _render(fb, sets, lv, points=points, sink=sink, K=8)
    if points_grad:
        torch.autograd.backward(list(o[:3]), [g_img[0], g_img[1], g_pts])
    else:
        torch.autograd.backward(list(o[:2]), list(g_img))
    torch.cuda.synchronize()
    d_feat = sink["points"] if how == "sink" else feat.grad
    return {**{k: (sink[k] if how == "sink" else lv[k].grad) for k in GEOM}, "track_gs": d_feat, "rgb": r.grad, "tap": fb.tap.clone()}


def _feature(per_frame):
    track_gs = _clip()[4]
    return track_gs if per_frame else track_gs[1].contiguous()


def _assert_bits(a, b, what, keys=None):
    for k in keys or a:
        if a[k] is None and b[k] is None:
            continue
        assert torch.equal(a[k], b[k]), f"{what}: d{k} differs"


# ------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("how", ["sink", "autograd"])
@pytest.mark.parametrize("per_frame", [True, False])
@pytest.mark.parametrize("kind", ["integer", "mixed"])
def test_ordered_batch_backward_matches_the_unordered_route(kind, per_frame, how):
    pts, counts = _queries(kind)
    off = _offsets(counts)
    g_pts = _t(np.random.default_rng(11).normal(size=(sum(counts), 3)))
    feature = _feature(per_frame)
    fb = FrameBatch(F, N, W, H, 4, "cuda")
    ref = _run(fb, False, feature, pts, off, g_pts, _image_grads(), how)
    got = _run(fb, True, feature, pts, off, g_pts, _image_grads(), how)
    assert got["track_gs"].shape == feature.shape
    _assert_doubled(got, ref, f"ordered vs unordered ({kind}, per_frame={per_frame}, {how})")
    # the sparse set's share alone (zero image gradients): every gradient is the ordered route's sum
    ref0 = _run(fb, False, feature, pts, off, g_pts, _image_grads(zero=True), how)
    got0 = _run(fb, True, feature, pts, off, g_pts, _image_grads(zero=True), how)
    _assert_doubled({k: got0[k] for k in SHARE}, {k: ref0[k] for k in SHARE}, "the sparse set's share alone")
    assert float(got0["opacity"].abs().max()) == 0


def test_a_query_no_frame_owns_contributes_nothing():
    pts, counts = _queries("integer")
    Q = sum(counts)
    off = _offsets(counts)
    bad = off.clone()
    bad[F] = Q - 7                      # the last 7 queries belong to nobody
    g_pts = _t(np.random.default_rng(12).normal(size=(Q, 3)))
    feature = _feature(True)
    fb = FrameBatch(F, N, W, H, 4, "cuda")
    zero = _image_grads(zero=True)
    a = _run(fb, True, feature, pts, bad, g_pts, zero)
    b = _run(fb, True, feature, pts[:Q - 7].contiguous(), bad, g_pts[:Q - 7].contiguous(), zero)
    full = _run(fb, True, feature, pts, off, g_pts, zero)
    _assert_bits(a, b, "orphan queries")
    assert not torch.equal(a["track_gs"], full["track_gs"])        # (they do count where a frame owns them)


# ------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("per_frame", [True, False])
def test_ordered_batch_backward_is_bit_reproducible(per_frame):
    pts, counts = _queries("mixed")
    ipts, icounts = _queries("integer")
    # both kinds of queries in one batch, frame by frame
    o_m, o_i = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum(icounts)])
    pts = torch.cat([t for f in range(F) for t in (pts[o_m[f]:o_m[f + 1]], ipts[o_i[f]:o_i[f + 1]])])
    counts = [a + b for a, b in zip(counts, icounts)]
    off = _offsets(counts)
    g_pts = _t(np.random.default_rng(13).normal(size=(sum(counts), 3)))
    feature = _feature(per_frame)
    fb = FrameBatch(F, N, W, H, 4, "cuda")
    zero = _image_grads(zero=True)
    runs = [_run(fb, True, feature, pts, off, g_pts, zero) for _ in range(3)]
    assert all(float(runs[0][k].abs().max()) > 0 for k in SHARE)
    L.set_deterministic(True)
    try:
        flagged = _run(fb, True, feature, pts, off, g_pts, zero)
        whole = [_run(fb, True, feature, pts, off, g_pts, _image_grads()) for _ in range(2)]
    finally:
        L.set_deterministic(False)
    for r in runs[1:]:
        _assert_bits(runs[0], r, "run to run")
    _assert_bits(runs[0], flagged, "under the deterministic flag")
    _assert_bits(whole[0], whole[1], "the whole backward under the deterministic flag")


# ------------------------------------------------------------------------------------------------------------- unchanged
def test_what_the_ordered_route_does_not_add_to_keeps_its_bits():
    pts, counts = _queries("integer")
    off = _offsets(counts)
    g_pts = _t(np.random.default_rng(14).normal(size=(sum(counts), 3)))
    feature = _feature(True)
    fb = FrameBatch(F, N, W, H, 4, "cuda")
    L.set_deterministic(True)            # (every kernel of the image backward is then reproducible too)
    try:
        with_pts = _run(fb, True, feature, pts, off, g_pts, _image_grads())
        none_grad = _run(fb, True, feature, pts, off, g_pts, _image_grads(), points_grad=False)
        # no sparse set at all
        clock, p, extr, rgb, track_gs, _, _ = _clip()
        lv = _leaves()
        r = rgb.clone().requires_grad_(True)
        o = _render(fb, [dict(feature=r, bg=0.2, taps=True), dict(feature="depth", bg=1.0)], lv, K=8)
        torch.autograd.backward(list(o[:2]), list(_image_grads()))
        plain = {**{k: lv[k].grad for k in GEOM}, "rgb": r.grad, "tap": fb.tap.clone()}
    finally:
        L.set_deterministic(False)
    # the sparse gradient adds to the geometry fields of the pair records and to the sparse feature: not to the taps, not to rgb
    _assert_bits(with_pts, plain, "with the sparse gradient", keys=["rgb", "tap"])
    assert all(not torch.equal(with_pts[k], plain[k]) for k in SHARE[:-1])
    # a None gradient of the sparse output launches nothing
    _assert_bits(none_grad, plain, "None gradient", keys=list(GEOM) + ["rgb", "tap"])
    assert float(none_grad["track_gs"].abs().max()) == 0
