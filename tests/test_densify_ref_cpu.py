"""The references of tests/densify_ref.py held to what they restate: the counter-based generator to its published vectors,
the float32 restatements to the derived bars, the float64 decisions and children to the C oracle / the numpy restatement of
the structure surgery (which tests/test_densify_cpu.py pins to the reference's own vectors)."""
import json
import os

import numpy as np
import pytest

import densify_ref as dr
import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
PROFILE = os.path.join(HERE, "..", "profiles", "densify_reference_cpu_float32.json")
SEEDS = (0, 77, 2 ** 32 + 5, 2 ** 64 - 1)


# ---------------------------------------------------------------------------------------------------------------------
def test_philox_reproduces_the_published_vectors():
    """the known-answer vectors of the generator's reference implementation (Random123, kat_vectors: philox4x32 10)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert philox_hex(dr.philox4x32_10(ctr, key)) == philox_hex(want)
        got = dr.philox4x32_10_np(*[np.array([c]) for c in ctr], *key)
        assert philox_hex(int(g[0]) for g in got) == philox_hex(want)
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, size=(4, 64), dtype=np.uint64)
    k0, k1 = 0x9abcdef0, 0x12345678
    got = np.stack(dr.philox4x32_10_np(*c, k0, k1), -1)
    for j in range(64):
        assert tuple(int(v) for v in got[j]) == dr.philox4x32_10(tuple(int(v) for v in c[:, j]), (k0, k1))


def philox_hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_u01_rounds_as_the_kernel_does():
    """[2^-25, 1], both ends reached: the +0.5 is lost to ties-to-even from x >> 8 = 2^23 on"""
    u = dr.u01(np.array([dr.U01_ONE, dr.U01_MIN, 0xFFFFFE00, 0x80000000, 0x80000100, 0x7FFFFF00], np.uint64))
    assert u.dtype == np.float32
    assert u[0] == np.float32(1.0) and u[1] == np.float32(2.0 ** -25)
    assert u[2] == np.float32((2 ** 24 - 2) * 2.0 ** -24)               # even: the half is dropped
    assert u[3] == np.float32(0.5) and u[4] == np.float32((2 ** 23 + 2) * 2.0 ** -24)      # 2^23 + 1.5 ties up to the even 2^23 + 2
    assert u[5] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)             # below 2^23 the half is exact
    z, r = dr.normals_ref([0], 1, 0)
    assert np.isfinite(z).all()
    assert np.sqrt(-2.0 * np.log(np.float64(dr.u01(dr.U01_ONE)))) == 0.0 and np.isfinite(np.log(np.float64(dr.u01(dr.U01_MIN))))


def test_draws_depend_on_both_seed_words_and_on_nothing_but_index_and_replica():
    idx = np.arange(300)
    z = {s: dr.normals_ref(idx, 3, s)[0] for s in SEEDS + (5, 2 ** 32 - 1)}
    assert not np.array_equal(z[2 ** 32 + 5], z[5]) and not np.array_equal(z[2 ** 64 - 1], z[2 ** 32 - 1])
    sub = np.array([3, 17, 299])
    assert np.array_equal(dr.normals_ref(sub, 3, 77)[0], z[77][sub])
    assert np.array_equal(dr.normals_ref(idx, 2, 77)[0], z[77][:, :2])
    allz = np.concatenate([dr.normals_ref(np.arange(20000), 2, s)[0].reshape(-1, 3) for s in SEEDS])
    assert abs(allz.mean()) < 5e-3 and abs(allz.std() - 1.0) < 5e-3 and abs((allz[:, 0] * allz[:, 1]).mean()) < 5e-3


# ---------------------------------------------------------------------------------------------------------------------
def envelope():
    """worst error / bar of the float32 numpy restatements over every children case and seed"""
    pos = scl = val = 0.0
    for N in dr.CHILD_N:
        for s in dr.CHILD_SPLIT:
            for kind in dr.CHILD_MASKS:
                c = dr.children_case(N, s, kind)
                a = (c["position"], c["scaling_raw"], c["rotation_raw"], c["mask"], s, c["normals"])
                rp, rs, rv = dr.children_ratios(*dr.children_f32(*a), dr.children_ref(*a))
                pos, scl, val = max(pos, rp), max(scl, rs), max(val, rv)
    idx = np.arange(5000)
    nrm = max(dr.normals_ratio(dr.normals_f32(idx, 3, s), idx, 3, s) for s in SEEDS)
    return {"children.pos": pos, "children.scl": scl, "children.pos_against_entry_values": val, "normals": nrm}


@pytest.fixture(scope="module")
def env():
    return envelope()


def test_float32_restatements_stay_inside_the_bars_and_the_envelope_file_is_current(env):
    print({k: float(f"{v:.4g}") for k, v in env.items()})
    for k in ("children.pos", "children.scl", "normals"):
        assert 0 < env[k] <= 1.0, (k, env[k])
    with open(PROFILE) as f:
        rec = json.load(f)
    assert rec["backend"] == "numpy_float32"
    assert rec["constants"] == dict(K_POS=dr.K_POS, K_SCL=dr.K_SCL, K_BM=dr.K_BM, MULT=dr.MULT, EXCLUDE_CAP=dr.EXCLUDE_CAP)
    for k, v in env.items():                          # (the libm behind numpy may move a worst case by an ulp)
        assert abs(rec["envelope"][k] - v) <= 0.25 * v, (k, rec["envelope"][k], v)


def test_committed_gpu_measurements_are_inside_the_bars():
    with open(os.path.join(HERE, "..", "profiles", "densify_reference_gpu.json")) as f:
        rec = json.load(f)
    assert rec["backend"] == "hip" and len(rec["build_id"]) == 16
    assert rec["constants"] == dict(K_POS=dr.K_POS, K_SCL=dr.K_SCL, K_BM=dr.K_BM, MULT=dr.MULT, EXCLUDE_CAP=dr.EXCLUDE_CAP)
    w = rec["worst"]
    ratios = [w["children"]["pos"], w["children"]["scl"], *w["generator"].values(), *w["statistics"].values(),
              *[v for r in w["train_step_children"].values() for v in r.values()]]
    assert len(ratios) >= 16 and all(0 < r <= 1.0 for r in ratios), ratios
    assert sorted(w["masks"]) == sorted(f"{p}.N{N}" for N in dr.MASK_N for p in dr.MASK_PARAMS)
    for case in w["masks"].values():
        for k in ("clone", "split", "prune"):
            assert case[k]["differ_where_compared"] == 0 and case[k]["left_out_share"] <= dr.EXCLUDE_CAP


def test_position_bar_needs_the_entries_operands(env):
    """with |R_kj| as the magnitude of an entry the bar is out of reach of float32: q / |q| is rounded before x y - r z is
    formed, so an entry the subtraction cancels keeps an absolute error of the size of its operands' roundings"""
    assert env["children.pos_against_entry_values"] > 1.0 > env["children.pos"]


# ---------------------------------------------------------------------------------------------------------------------
CASES = [(N, p) for N in dr.MASK_N for p in dr.MASK_PARAMS]


@pytest.mark.parametrize("N,params", CASES)
def test_oracle_masks_agree_on_every_clear_and_tie_row(oracle_mod, N, params):
    c = dr.mask_case(N, params)
    got = oracle_mod.densify_masks(c["accum"], c["denom"], c["max_radii2D"], c["scaling_raw"], c["opacity_raw"], *c["args"])
    for k, a in zip(("clone", "split", "prune"), got):
        rows = dr.compared_rows(c, k)
        left_out = int((~rows).sum())
        print(c["id"], k, "left out", left_out, "of", N)
        assert left_out <= int(dr.EXCLUDE_CAP * N), (c["id"], k, left_out)
        assert np.array_equal(a[rows], c["ref"][k][rows]), (c["id"], k, np.flatnonzero(rows & (a != c["ref"][k]))[:10])


def test_mask_strata_are_what_they_claim():
    m = dr.MULT * dr.EPS32
    for params in dr.MASK_PARAMS:
        c = dr.mask_case(257, params)
        ref, st = c["ref"], c["stratum"]
        assert all(int((st == k).sum()) > 0 for k in range(4))
        near = st == dr.STRATA.index("near")
        d = np.stack([ref["dist"][k] for k in ("grad_abs", "dense", "big_ws", "min_opacity", "size")], 1)
        assert all(ref["clear"][k][near].all() for k in ref["clear"])
        if c["args"][4] > 0:
            assert (np.abs(d[near].min(1) - 1e-4) < 2e-6).all()            # every near row sits 1e-4 from one threshold
            assert sorted(set(d[near].argmin(1))) == [0, 1, 2, 3, 4]        # and every threshold has its rows
        tie = np.flatnonzero(st == dr.STRATA.index("tie"))
        for k in ("grad_abs", "grad", "dense", "big_ws", "min_opacity", "size"):
            assert ((ref["dist"][k][tie] == 0) | (ref["dist"][k][tie] > m)).all(), (params, k)      # exact, or clear
    c = dr.mask_case(257, "ties")
    ref = c["ref"]
    a, b, o, r = _tie_rows(c)
    assert ref["dist"]["grad"][a] == 0 and ref["dist"]["dense"][a] == 0 and ref["clone"][a] and not ref["split"][a]
    assert ref["dist"]["grad"][b] == 0 and ref["split"][b] and not ref["clone"][b]
    assert ref["dist"]["min_opacity"][o] == 0 and not ref["prune"][o]
    assert ref["dist"]["size"][r] == 0 and not ref["prune"][r]
    # size_threshold = 0: no radius and no scale prunes
    c = dr.mask_case(257, "nosize")
    assert np.array_equal(c["ref"]["prune"], c["ref"]["opac"] < np.float64(c["th"]["min_opacity"]))
    assert (c["max_radii2D"][~c["ref"]["prune"]] > 100).any() and (c["ref"]["smax"][~c["ref"]["prune"]] > 3.5e38).any()


def _tie_rows(c):
    """the four tie rows in the order _deliberate_rows lists them (found by their values)"""
    tie = np.flatnonzero(c["stratum"] == dr.STRATA.index("tie"))
    sc, op, mr = c["scaling_raw"], c["opacity_raw"].reshape(-1), c["max_radii2D"]
    a = next(i for i in tie if (sc[i] == 0).all())
    b = next(i for i in tie if sc[i, 0] == 3.0)
    o = next(i for i in tie if op[i] == 0.0)
    r = next(i for i in tie if mr[i] == c["th"]["size"] and op[i] == 5.0)
    return a, b, o, r


# ---------------------------------------------------------------------------------------------------------------------
def test_statistics_restatement_is_the_oracle():
    """StatsRef against the C oracle's accumulate / update (itself pinned to the reference's vectors): the linear outputs bit
    for bit, the accumulated norm within the existing bar"""
    N, F = 3001, 3
    ref = dr.StatsRef(N)
    vg = np.zeros((N, 2), np.float32); vis = np.zeros(N, np.uint8); rr = np.zeros(N, np.int32)
    mr = np.zeros(N, np.float32); acc = np.zeros(N, np.float32); den = np.zeros(N, np.float32)
    for step in range(3):
        ref.begin_batch()
        vg[...] = 0; vis[...] = 0; rr[...] = 0
        for radius, tap in dr.stats_frames(N, F, step):
            ref.accumulate_frame(radius, tap, dr.STATS_SCALE)
            oracle.densify_accumulate(radius, tap, *dr.STATS_SCALE, vg, vis, rr)
        assert np.array_equal(ref.viewspace_grad, vg) and np.array_equal(ref.visibility, vis) and np.array_equal(ref.radii, rr)
        ref.update()
        oracle.densify_update(vis, vg, rr, mr, acc, den)
        assert np.array_equal(ref.max_radii2D, mr) and np.array_equal(ref.denom, den)
        np.testing.assert_allclose(acc, ref.accum64, rtol=2e-6, atol=0)
        np.testing.assert_allclose(ref.pos_gradient_accum, ref.accum64, rtol=2e-6, atol=0)
    assert 0 < int(vis.sum()) < N and (rr == 0).any()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split_num", dr.CHILD_SPLIT)
def test_oracle_structure_surgery_agrees_with_the_children_reference(split_num):
    rng = np.random.default_rng(split_num)
    for N, kind in ((1, "all"), (257, "random"), (257, "none"), (5000, "random"), (5000, "last")):
        c = dr.children_case(N, split_num, kind)
        names = {"position": c["position"], "scaling": c["scaling_raw"], "rotation": c["rotation_raw"],
                 "opacity": rng.normal(size=(N, 1)).astype(np.float32), "features": rng.normal(size=(N, 4, 3)).astype(np.float32)}
        mom = {k: (rng.normal(size=v.shape).astype(np.float32), rng.uniform(size=v.shape).astype(np.float32)) for k, v in names.items()}
        p1, m1 = oracle.structure_clone(names, mom, c["mask"])
        q1, n1 = dr.clone_np(names, mom, c["mask"])
        for k in names:
            assert np.array_equal(p1[k], q1[k]) and all(np.array_equal(a, b) for a, b in zip(m1[k], n1[k]))
        p2, m2, new_pos, new_scl = oracle.structure_split(names, mom, c["mask"], split_num, c["normals"])
        ref = dr.children_ref(c["position"], c["scaling_raw"], c["rotation_raw"], c["mask"], split_num, c["normals"])
        rp, rs, _ = dr.children_ratios(new_pos, new_scl, ref)
        assert rp <= 1.0 and rs <= 1.0, (c["id"], rp, rs)
        q2, n2, valid = dr.split_np(names, mom, c["mask"], split_num, new_pos, new_scl)
        for k in names:
            assert np.array_equal(p2[k], q2[k]) and all(np.array_equal(a, b) for a, b in zip(m2[k], n2[k]))
        assert int(valid.sum()) == N + (split_num - 1) * c["n"]
