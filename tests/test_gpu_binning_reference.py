"""Tile binning + per-tile sort (csrc/binning.hip) against tests/binning_ref.py -- numpy, vectorised, independent of the C
oracle's loop order -- on every branch of the host's plan: the LDS and the global-atomic path, the last LDS size, the row cap,
both trips of the tile scan, upper row groups of the column scan, the natural fall-back to slot keys, every size class and
class boundary of the per-tile sort, frame-batch chunking, the edges of the rectangle rule, capacity overflow, and reach masks
and one render on both sides of the LDS / global boundary.  Every expected value is an integer: every comparison is exact.

The library is called two ways: through gs.sort_gaussian / gs.sort_gaussian_capped (pair-map mode: goff_incl, slot_sorted) and
through the raw C ABI with goff_incl / owner / slot_sorted NULL (low key word = Gaussian id)."""

import numpy as np
import pytest
import torch

import binning_ref as R
import splatter_a_video_amd._lib as L

pytestmark = pytest.mark.gpu

SENT = -7   # prefill of every output buffer: what the library did not write still holds it


def _t(a, grad=False):
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return t.requires_grad_() if grad else t


def _n(t):
    return t.detach().cpu().numpy()


def _full(n, dtype=torch.int32):
    return torch.full((int(n),), SENT, dtype=dtype, device="cuda")


def _pairmap_sort(uv, depth, radius, W, H):
    import dptr.gs as gs
    idx, tr, st = gs.sort_gaussian_capped(uv, depth, W, H, radius, None)
    torch.cuda.synchronize()
    return dict(idx=_n(idx), tr=_n(tr), M=int(st.pairs.item()), goff=_n(st.pairmap.goff), slot=_n(st.pairmap.slot_sorted))


def _raw_sort(uv, depth, radius, W, H, capacity=None, pairmap=False, extra=0):
    """splat_bin_count + splat_bin_sort; capacity: None (= M) or a function of M; buffers hold max(M, capacity) + extra entries"""
    lib, st = L.lib(), L.stream()
    P = radius.numel()
    gx, gy = R.grid(W, H)
    scratch = torch.empty(lib.splat_bin_scratch_bytes(P, W, H), dtype=torch.uint8, device="cuda")
    tr, m, gcount = _full(2 * gx * gy).view(-1, 2), _full(1), _full(P)
    L.check(lib.splat_bin_count(P, L.ptr(uv), L.ptr(radius), W, H, L.ptr(scratch), L.ptr(tr), L.ptr(m), L.ptr(gcount), st))
    M = int(m.item())
    cap = M if capacity is None else int(capacity(M))
    n = max(M, cap) + extra
    keys, idx, ovf = _full(n, torch.int64), _full(n), torch.zeros(1, dtype=torch.int32, device="cuda")
    goff, owner, slot = (_full(P), _full(n), _full(n)) if pairmap else (None, None, None)
    L.check(lib.splat_bin_sort(P, L.ptr(uv), L.ptr(depth), L.ptr(radius), W, H, L.ptr(scratch), L.ptr(tr),
                               cap, L.ptr(keys), L.ptr(idx), L.ptr(ovf), L.ptr(goff), L.ptr(owner), L.ptr(slot), st))
    torch.cuda.synchronize()
    out = dict(idx=_n(idx), tr=_n(tr), M=int(m.item()), gcount=_n(gcount), ovf=int(ovf.item()), cap=cap, keys=_n(keys))
    if pairmap:
        out.update(goff=_n(goff), owner=_n(owner), slot=_n(slot))
    return out


def _assert_equal(got, ref, what):
    assert got["M"] == ref.M, what
    assert np.array_equal(got["tr"], ref.tile_range), what
    assert np.array_equal(got["idx"][:ref.M], ref.idx_sorted), what
    if "gcount" in got:
        assert np.array_equal(got["gcount"], ref.gcount), what
    if "goff" in got:
        assert np.array_equal(got["goff"], ref.goff_incl), what
        assert np.array_equal(got["slot"][:ref.M], ref.slot_sorted), what
    if "ovf" in got:
        assert got["ovf"] == 0, what


def _both_ways(uv, depth, radius, W, H, ref, what):
    d = (_t(uv), _t(depth), _t(radius))
    _assert_equal(_pairmap_sort(*d, W, H), ref, what + ": pair-map mode")
    raw = _raw_sort(*d, W, H, extra=64)
    _assert_equal(raw, ref, what + ": raw ABI")
    assert (raw["idx"][ref.M:] == SENT).all() and (raw["keys"][ref.M:] == SENT).all(), what


# ------------------------------------------------------------------ (a) plan branches
@pytest.mark.parametrize("case", R.PLAN_CASES, ids=lambda c: c.name)
def test_plan_branches(gpu, case):
    uv, depth, radius = R.case_inputs(case)
    _both_ways(uv, depth, radius, case.W, case.H, R.case_reference(case.name), case.name + " (" + case.branch + ")")


# ------------------------------------------------------------------ (b) every list length on purpose
@pytest.mark.parametrize("slot_keys", [0, 1])
@pytest.mark.parametrize("pattern", R.DEPTH_PATTERNS)
def test_every_list_length(gpu, lib_option, pattern, slot_keys):
    """one tile per length: the four size classes of tile_sort_kernel, their boundaries, the wave-live boundaries (multiples of
    64 R) and crowded lengths on both sides of whole 2048-key blocks and of powers of two"""
    lib_option("bin_slot_keys", slot_keys)
    uv, depth, radius, W, H, _ = R.length_inputs(pattern)
    ref = R.length_reference(pattern)
    assert (ref.tile_range[:, 1] - ref.tile_range[:, 0]).tolist() == R.LIST_LENGTHS
    _both_ways(uv, depth, radius, W, H, ref, f"{pattern}, bin_slot_keys {slot_keys}")
    pm = _raw_sort(_t(uv), _t(depth), _t(radius), W, H, pairmap=True)
    _assert_equal(pm, ref, f"{pattern}, bin_slot_keys {slot_keys}: raw ABI with the pair map")
    if slot_keys:
        assert np.array_equal(pm["owner"], np.repeat(np.arange(radius.size), ref.gcount))


# ------------------------------------------------------------------ (c) rectangle edges
@pytest.mark.parametrize("W,H", [(77, 50), (16 * 12289, 16)], ids=["small", "T12289"])
def test_rectangle_edges(gpu, W, H):
    import dptr.gs as gs
    import dptr.gs._C as _C
    uv, depth, radius = R.edge_inputs(W, H)
    ref = R.sort(uv, depth, radius, W, H)
    gx, gy = R.grid(W, H)
    assert int((ref.gcount == gx * gy).sum()) == 3 and int(((radius > 0) & (ref.gcount == 0)).sum()) >= 6 and int((radius <= 0).sum()) >= 8
    _both_ways(uv, depth, radius, W, H, ref, "edges")
    d = (_t(uv), _t(depth), _t(radius))
    idx, tr = gs.sort_gaussian(d[0], d[1], W, H, d[2], _t(ref.gcount))
    assert np.array_equal(_n(idx), ref.idx_sorted) and np.array_equal(_n(tr), ref.tile_range)
    # the reference-flow helpers on the same inputs
    key, gid = _C.compute_gaussian_key(d[0], d[1], W, H, d[2], _t(ref.goff_incl))
    rkey, rgid = R.keys(uv, depth, radius, W, H)
    assert np.array_equal(_n(key), rkey) and np.array_equal(_n(gid), rgid)
    ks = np.sort(rkey, kind="stable")
    tr2 = _C.compute_tile_gaussian_range(W, H, None, _t(ks))
    assert np.array_equal(_n(tr2), ref.tile_range)


# ------------------------------------------------------------------ (d) frame batch
def _batch(F, P, W, H, rmax, seed):
    lib, st = L.lib(), L.stream()
    gx, gy = R.grid(W, H)
    T = gx * gy
    frames = [R.random_inputs(P, W, H, rmax, seed + 31 * f) for f in range(F)]
    refs = [R.sort(uv, depth, radius, W, H) for uv, depth, radius in frames]
    uv, depth, radius = (_t(np.stack([fr[k] for fr in frames])) for k in range(3))
    bytes_ = lib.splat_bin_scratch_bytes(P, W, H)
    scratch = torch.empty(F * bytes_, dtype=torch.uint8, device="cuda")
    tr, m = _full(F * T * 2).view(F, T, 2), _full(F)
    L.check(lib.splat_bin_count_batch(F, P, L.ptr(uv), L.ptr(radius), W, H, L.ptr(scratch), L.ptr(tr), L.ptr(m), st))
    Ms = _n(m).tolist()
    assert Ms == [r.M for r in refs]
    cap = max(Ms) + 100
    keys, idx, owner, slot = _full(F * cap, torch.int64), _full(F * cap), _full(F * cap), _full(F * cap)
    goff, ovf = _full(F * P), torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(lib.splat_bin_sort_batch(F, P, L.ptr(uv), L.ptr(depth), L.ptr(radius), W, H, L.ptr(scratch), L.ptr(tr),
                                     cap, L.ptr(keys), L.ptr(idx), L.ptr(ovf), L.ptr(goff), L.ptr(owner), L.ptr(slot), st))
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    tr, idx, slot, goff, keys, owner = _n(tr), _n(idx).reshape(F, cap), _n(slot).reshape(F, cap), _n(goff).reshape(F, P), \
        _n(keys).reshape(F, cap), _n(owner).reshape(F, cap)
    for f, ref in enumerate(refs):
        what = f"frame {f} of {F}, P {P}"
        assert np.array_equal(tr[f], ref.tile_range), what
        assert np.array_equal(idx[f, :ref.M], ref.idx_sorted), what
        assert np.array_equal(slot[f, :ref.M], ref.slot_sorted), what
        assert np.array_equal(goff[f], ref.goff_incl), what
        for name, a in (("idx_sorted", idx), ("slot_sorted", slot), ("keys", keys), ("owner", owner)):
            assert (a[f, ref.M:] == SENT).all(), (what, name)


@pytest.mark.parametrize("P", [2047, 2048, 2049, 5000])
@pytest.mark.parametrize("F", [1, 3, 4, 5])
def test_frame_batch_lds(gpu, F, P):
    """from BIN_BATCH_FRAMES frames on the batch uses BIN_CHUNK_BATCH chunks inside the single-frame scratch layout"""
    assert R.plan(P, 320, 240, F)["NB"] == (-(-P // 2048) if F >= 4 else -(-P // 512))
    _batch(F, P, 320, 240, 40, 1000 * F + P)


@pytest.mark.parametrize("F", [2, 4])
def test_frame_batch_global(gpu, F):
    _batch(F, 3000, 16 * 12289, 16, 200, 77 + F)


# ------------------------------------------------------------------ (e) overflow on both paths
@pytest.mark.parametrize("pairmap", [True, False], ids=["pairmap", "ids"])
@pytest.mark.parametrize("slot_keys", [0, 1])
@pytest.mark.parametrize("frac", ["half", "minus1"])
@pytest.mark.parametrize("W,H,rmax", [(320, 240, 40), (16 * 12289, 16, 200)], ids=["lds", "global"])
def test_overflow_is_flagged_and_stays_inside_the_capacity(gpu, lib_option, W, H, rmax, frac, slot_keys, pairmap):
    """every buffer holds M + 1024 entries, the library is told a smaller capacity: a missing clamp shows in the sentinels and
    cannot leave the allocation"""
    lib_option("bin_slot_keys", slot_keys)
    P = 3000
    uv, depth, radius = R.random_inputs(P, W, H, rmax, 4242)
    ref = R.sort(uv, depth, radius, W, H)
    capf = (lambda M: M // 2) if frac == "half" else (lambda M: M - 1)
    got = _raw_sort(_t(uv), _t(depth), _t(radius), W, H, capacity=capf, pairmap=pairmap, extra=1024)
    cap = got["cap"]
    assert 0 < cap < ref.M and got["idx"].size == ref.M + 1024
    assert got["ovf"] == 1 and got["M"] == ref.M and np.array_equal(got["gcount"], ref.gcount)
    tr = got["tr"]
    assert tr.max() <= cap and tr.min() >= 0 and (tr[:, 0] <= tr[:, 1]).all()
    assert np.array_equal(tr, np.minimum(ref.tile_range, cap))          # the clamp of tile_sort_kernel, entry by entry
    names = ["keys", "idx"] + (["owner", "slot"] if pairmap else [])
    for name in names:
        assert (got[name][cap:] == SENT).all(), name                     # nothing past the capacity was written
    assert (got["idx"][:cap] >= 0).all() and (got["idx"][:cap] < P).all()
    whole = ref.tile_range[:, 1] <= cap                                 # tiles that lie below the capacity: complete and sorted
    keep = np.repeat(whole, ref.tile_range[:, 1] - ref.tile_range[:, 0])
    n_keep = int(keep.sum())
    assert n_keep > 0 and keep[:n_keep].all()
    # (slot keys resolve the id through owner[slot]: a pair whose slot lies past the capacity has lost its id, by design)
    named = ref.slot_sorted[:n_keep] < cap if (pairmap and slot_keys) else np.ones(n_keep, bool)
    assert named.any() and np.array_equal(got["idx"][:n_keep][named], ref.idx_sorted[:n_keep][named])
    if pairmap:
        assert np.array_equal(got["goff"], np.minimum(ref.goff_incl, cap))
        assert (got["slot"][:cap] >= 0).all() and (got["slot"][:cap] < cap).all()
        assert np.array_equal(got["slot"][:n_keep], np.minimum(ref.slot_sorted[:n_keep], cap - 1))


# ------------------------------------------------------------------ (f) reach masks on the global path
def _reach_sort(d, W, H):
    lib, st = L.lib(), L.stream()
    uv, depth, radius, conic, op = d
    P = radius.numel()
    gx, gy = R.grid(W, H)
    scratch = torch.empty(lib.splat_bin_scratch_bytes(P, W, H), dtype=torch.uint8, device="cuda")
    tr, m, gcount, reach = _full(2 * gx * gy).view(-1, 2), _full(1), _full(P), _full(P)
    L.check(lib.splat_bin_count_batch_reach(1, P, L.ptr(uv), L.ptr(radius), L.ptr(conic), L.ptr(op), 0,
                                            W, H, L.ptr(scratch), L.ptr(tr), L.ptr(m), L.ptr(gcount), L.ptr(reach), st))
    M = int(m.item())
    keys, idx, owner, slot = _full(M, torch.int64), _full(M), _full(M), _full(M)
    goff, ovf = _full(P), torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(lib.splat_bin_sort_batch_reach(1, P, L.ptr(uv), L.ptr(depth), L.ptr(radius), L.ptr(reach), W, H,
                                           L.ptr(scratch), L.ptr(tr), M, L.ptr(keys), L.ptr(idx), L.ptr(ovf),
                                           L.ptr(goff), L.ptr(owner), L.ptr(slot), st))
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    return dict(M=M, tr=_n(tr), gcount=_n(gcount), reach=_n(reach), idx=_n(idx), slot=_n(slot), goff=_n(goff))


WA, WB, HR = 16 * R.REACH_GX, 16 * (R.REACH_GX + 1), 32


def _left(tr, gx):
    """tile ranges [gy, gx, 2] -> (columns left of REACH_GX, the rest)"""
    tr = tr.reshape(2, gx, 2)
    return tr[:, :R.REACH_GX], tr[:, R.REACH_GX:]


def test_reach_masks_agree_across_the_lds_boundary(gpu):
    """the same Gaussians on 6144 x 2 tiles (LDS path) and on 6145 x 2 tiles (global path), every rectangle left of column 6144"""
    inp = R.reach_inputs()
    uv, depth, radius, conic, op = inp
    assert R.plan(radius.size, WA, HR)["lds"] and not R.plan(radius.size, WB, HR)["lds"]
    d = tuple(_t(a) for a in inp)
    a, b = _reach_sort(d, WA, HR), _reach_sort(d, WB, HR)
    full = R.sort(uv, depth, radius, WA, HR)
    fullb = R.sort(uv, depth, radius, WB, HR)
    assert np.array_equal(full.gcount, fullb.gcount) and np.array_equal(full.idx_sorted, fullb.idx_sorted)
    # the scene holds what it is there for
    assert int((full.gcount >= 32).sum()) >= 40 and int((a["reach"] < 0).sum()) >= 40          # cell form of the reach word
    assert (a["gcount"] <= full.gcount).all() and int((a["gcount"][full.gcount >= 32] < full.gcount[full.gcount >= 32]).sum()) > 0
    faint = op < 1.0 / 255.0
    assert int(faint.sum()) == 300 and int(full.gcount[faint].sum()) > 0 and int(a["gcount"][faint].sum()) == 0
    assert 0 < a["M"] < full.M
    # identical across the two grids
    for k in ("reach", "gcount", "M", "goff", "idx", "slot"):
        assert np.array_equal(a[k], b[k]), k
    la, ra = _left(a["tr"], R.REACH_GX)
    lb, rb = _left(b["tr"], R.REACH_GX + 1)
    assert np.array_equal(la, lb) and ra.size == 0 and not rb.any()
    # against the reference: counts, prefix, and every kept list a sub-sequence, in order, of the full list
    assert a["M"] == int(a["gcount"].sum()) and np.array_equal(a["goff"], np.cumsum(a["gcount"]))
    P = radius.size
    cnt = (a["tr"][:, 1] - a["tr"][:, 0]).astype(np.int64)
    assert int(cnt.sum()) == a["M"] and np.array_equal(a["tr"][cnt > 0, 1], np.cumsum(cnt)[cnt > 0])
    key = np.repeat(np.arange(cnt.size, dtype=np.int64), cnt) * P + a["idx"]
    fkey = full.tile_sorted * P + full.idx_sorted
    order = np.argsort(fkey, kind="stable")
    pos = order[np.minimum(np.searchsorted(fkey[order], key), fkey.size - 1)]
    assert np.array_equal(fkey[pos], key) and (np.diff(pos) > 0).all()
    # slot_sorted names the owner
    assert np.array_equal(np.sort(a["slot"]), np.arange(a["M"]))
    assert np.array_equal(np.repeat(np.arange(P), a["gcount"])[a["slot"]], a["idx"])


# ------------------------------------------------------------------ (g) one render across the boundary
@pytest.mark.parametrize("reach", [False, True], ids=["full", "reach"])
def test_render_across_the_lds_boundary(gpu, reach):
    import dptr.gs as gs
    import dptr.gs._C as _C
    from test_gpu_parity import assert_grad
    uv, depth, radius, conic, op = R.reach_inputs()
    P, C, bg = radius.size, 3, 0.2
    rng = np.random.default_rng(3)
    feat = rng.uniform(size=(P, C)).astype(np.float32)
    g = rng.normal(size=(C, HR, WB)).astype(np.float32)
    res = []
    for W in (WA, WB):
        p = dict(uv=_t(uv, True), conic=_t(conic, True), opacity=_t(op, True), feature=_t(feat, True))
        with torch.no_grad():
            extra = (p["conic"], p["opacity"]) if reach else ()
            idx, tr, st = gs.sort_gaussian_capped(p["uv"], _t(depth), W, HR, _t(radius), None, *extra)
        img = gs.alpha_blending(p["uv"], p["conic"], p["opacity"], p["feature"], idx, tr, bg, W, HR)
        img.backward(_t(g[:, :, :W]))
        with torch.no_grad():
            _, final_T, ncontrib = _C.alpha_blending_forward(p["uv"], p["conic"], p["opacity"], p["feature"], idx, tr, bg, W, HR)
        torch.cuda.synchronize()
        res.append((img.detach()[:, :, :WA].cpu(), final_T[:, :WA].cpu(), ncontrib[:, :WA].cpu(), {k: _n(v.grad) for k, v in p.items()},
                    img.detach()[:, :, WA:].cpu(), st.check()))
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[5] == b[5] and int(a[2].max()) > 3 and float(a[1].min()) < 0.5        # lists of several splats, opaque pixels
    assert bool((b[4] == bg).all())                                                 # nothing reaches the extra tile column
    for k in a[3]:
        assert np.abs(b[3][k]).max() > 0
        assert_grad(a[3][k], b[3][k], k)
