"""The test of the frame batch's Gaussian-side backward (tests/test_gpu_gauss_backward_reference.py) proven on the CPU: the
record builder's invariants (prefixes, poison, sums exact in float32 in any order), the count tables, which rows receive
records, and the float32 C oracle's operator chain fed the same record sums -- it must lie inside the bars the HIP kernels
are held to, on every row (tests/gauss_backward_ref.py)."""
import json
import os

import numpy as np
import pytest

import gauss_backward_ref as gb
import geometry_ref as gr

HERE = os.path.dirname(os.path.abspath(__file__))
LAYOUTS = {"plain8": lambda: gb.plain_layout(1, False), "plain12abs": lambda: gb.plain_layout(3, True),
           "plain40abs": lambda: gb.plain_layout(32, True), "sets16": lambda: gb.sets_layout(2),
           "sets36": lambda: gb.sets_layout(23)}


@pytest.mark.parametrize("P", gb.LINEAR_P)
@pytest.mark.parametrize("F", gb.LINEAR_F)
def test_count_table(F, P):
    cnt = gb.count_table(F, P)
    i = np.arange(P)
    edge = (i % 64 == 0) | (i % 64 == 63) | (i == P - 1)
    assert (cnt[:, edge] > 0).all(), "the first and last Gaussian of every block of 64 own a record in every frame"
    assert cnt.sum(0).max() < 2 ** 14
    if P >= 63:
        assert (cnt[:, gb.ZERO_ROW] == 0).all() and (cnt == gb.LONG).sum() == 2 and (cnt[F - 1] == gb.LONG).any()
        assert set(gb.CYCLE) <= set(np.unique(cnt).tolist())
    if F >= 33:
        assert ((cnt[32:] > 0).mean(1) >= 0.5).all(), "frames past the LDS table carry records for half the rows"


@pytest.mark.parametrize("lkey", sorted(LAYOUTS))
@pytest.mark.parametrize("F,P", [(1, 1), (3, 65), (34, 257)])
def test_builder_invariants(F, P, lkey):
    lay = LAYOUTS[lkey]()
    cnt = gb.count_table(F, P)
    R = gb.build_records(cnt, lay, seed=1)
    goff, cap, rec = R["goff"], R["cap"], R["rec"]
    assert rec.shape == (F, cap, lay["stride"]) and rec.dtype == np.float32 and goff.dtype == np.int32
    assert (np.diff(goff, axis=1) >= 0).all() and (goff[:, 0] >= 0).all() and (goff[:, -1] <= cap - gb.SLACK).all()
    assert (np.diff(np.concatenate([np.zeros((F, 1), np.int32), goff], 1), axis=1) == cnt).all()
    pad = sorted(set(range(lay["stride"])) - set(lay["used"]))
    if lay["kind"] == "sets":
        assert 10 in pad and 11 in pad
    for f in range(F):
        n = goff[f, -1]
        assert np.isnan(rec[f, n:]).all(), "unowned slots are poisoned"
        assert np.isnan(rec[f, :n][:, pad]).all(), "padding floats are poisoned"
        v = rec[f, :n][:, lay["used"]].astype(np.float64) * 256
        assert (v == np.round(v)).all() and (np.abs(v) <= 256).all()
        if lay["nonneg"]:
            assert (rec[f, :n][:, lay["nonneg"]] >= 0).all()
    # a float32 sequential sum in three orders equals the float64 sum bit for bit
    S = gb.segment_sums(R).sum(0)[:, lay["used"]]
    rng = np.random.default_rng(0)
    for i in range(P):
        mine = np.concatenate([rec[f][R["owner"][f] == i][:, lay["used"]] for f in range(F)])
        if not len(mine):
            assert (S[i] == 0).all()
            continue
        for order in (np.arange(len(mine)), np.arange(len(mine))[::-1], rng.permutation(len(mine))):
            seq = np.cumsum(mine[order], axis=0, dtype=np.float32)[-1]
            assert seq.dtype == np.float32
            np.testing.assert_array_equal(seq.astype(np.float64), S[i])


def test_strides_are_complete():
    """plain records reach every stride the library hands out for them and SETS records every stride from 16 (their twelve
    geometry floats and one channel) to 40; together all nine instantiated strides 8 .. 40"""
    from test_gpu_gauss_backward_reference import PLAIN_CONFIGS, SETS_CS
    plain = {gb.plain_layout(C, a)["stride"] for C, a in PLAIN_CONFIGS}
    sets = {gb.sets_layout(C)["stride"] for C in SETS_CS}
    assert sorted(plain) == gb.plain_strides() == [8, 12, 16, 24, 28, 32, 40]
    assert sorted(sets) == gb.sets_strides() == [16, 20, 24, 28, 32, 36, 40]
    assert sorted(plain | sets) == list(range(8, 41, 4))
    assert 23 in SETS_CS


@pytest.mark.parametrize("cam", sorted(gb.CHAIN_CAMS))
@pytest.mark.parametrize("F", gb.CHAIN_F)
def test_rows_that_receive_records(F, cam):
    e = gb.static_eligibility(gb.CHAIN_CAMS[cam], F, cam)
    assert e.any(0).mean() >= 0.25
    c = gr.case_by_id(gb.CHAIN_CAMS[cam])
    # (rows behind the FIRST camera or at its tz == 0 come into view of the later cameras; one camera never sees them)
    for kind in ("behind", "tz0", "nonfinite") if cam == 0 else ("nonfinite",):
        assert not e[:, c["edge_kind"] == kind].any()
        assert not e[0][c["edge_kind"] == kind].any()
    if F >= 33:
        assert (e[32:].mean(1) >= 0.25).all()


@pytest.mark.parametrize("name", sorted(gb.DYN_TIMES))
def test_dynamic_rows_that_receive_records(name):
    e = gb.dyn_eligibility(name)
    assert e.any(0).mean() >= 0.25
    assert e[:, list(gb.DYN_HARD_ROWS)].any(0).all(), "the rows with the hard quaternions / logits own records"
    P = gb.dyn_problem(name, "plain_narrow")
    assert (P["R"]["cnt"][:, list(gb.DYN_HARD_ROWS)].sum(0) > 0).all()
    segs = gb.segments(gb.dyn_case(), gb.DYN_TIMES[name])
    if name == "segments_ABA":
        assert segs[0] == segs[-1] != segs[2] and len(set(segs)) == 2
    if name.startswith("run"):
        assert len(set(segs)) == 1 and len(segs) == int(name[3:])


REPORTS = []


@pytest.mark.parametrize("lkey", ["plain_narrow", "sets_wide"])
@pytest.mark.parametrize("cam", sorted(gb.CHAIN_CAMS))
@pytest.mark.parametrize("F", gb.CHAIN_F)
def test_oracle_static_chain_meets_the_bars(oracle_mod, F, cam, lkey):
    P = gb.static_problem(F, cam, lkey)
    rep = gr.Report(P["c"])
    gb.check_chain(rep, "", gb.oracle_static(oracle_mod, P["frames"], P["R"], P["S"], P["depth_channel"]), P["ref"])
    REPORTS.append(rep)
    rep.finish()


@pytest.mark.parametrize("lkey", ["plain_narrow", "sets_wide"])
@pytest.mark.parametrize("name", sorted(gb.DYN_TIMES))
def test_oracle_dynamic_chain_meets_the_bars(oracle_mod, name, lkey):
    P = gb.dyn_problem(name, lkey)
    rep = gr.Report(P["c"])
    gb.check_chain(rep, "", gb.oracle_dynamic(oracle_mod, gb.dyn_case(), P["times"], P["R"], P["S"], P["depth_channel"]), P["ref"])
    REPORTS.append(rep)
    rep.finish()


def test_committed_measurements_are_inside_the_bars():
    for name, backend in (("gauss_backward_reference_cpu_float32.json", "oracle"), ("gauss_backward_reference_gpu.json", "hip")):
        with open(os.path.join(HERE, "..", "profiles", name)) as f:
            rec = json.load(f)
        assert rec["backend"] == backend and 0 < rec["worst_overall"] <= 1.0
        assert rec["constants"] == dict(KAPPA0=gr.KAPPA0, WIDEN_SLOPE=gr.WIDEN_SLOPE, KAPPA_DEAD=gr.KAPPA_DEAD)
