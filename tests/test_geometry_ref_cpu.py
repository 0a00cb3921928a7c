"""The float32 C oracle held to the float64 twin on the hard cases of tests/geometry_ref.py, at exactly the bars the HIP
kernels are held to (tests/test_gpu_geometry_reference.py): this is what proves those bars attainable in float32, and it
replaces the 250-Gaussian relative-to-maximum link between the oracle and the twin by a per-row one.  Also: gradcheck of
the extended twin, the dynamic twin against the reference's own vectors, and the exclusion caps from the float64 side."""
import json
import os

import numpy as np
import pytest
import torch

import geometry_ref as gr
import torch_twin as tw

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("cid", gr.CASE_IDS)
def test_oracle_operators_meet_the_bars(oracle_mod, cid):
    c = gr.case_by_id(cid)
    rep = gr.Report(c)
    r, e, masks = gr.run_operators(gr.OracleBackend(oracle_mod), c, rep)
    rep.finish()
    gr.assert_caps(c, masks)
    gr.assert_bounds_populated(c, r)
    assert gr.conditioned_share(e) >= 0.95


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("cid", gr.CASE_IDS)
def test_oracle_chain_meets_the_bars(oracle_mod, cid, offset):
    c = gr.case_by_id(cid)
    rep = gr.Report(c)
    r, masks = gr.run_fused(gr.OracleBackend(oracle_mod), c, rep, offset)
    rep.finish()
    gr.assert_caps(c, masks)
    assert gr.conditioned_share(r) >= 0.95


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_oracle_sh_meets_the_bars(oracle_mod, deg, free):
    c = gr.make_sh_case(deg)
    rep = gr.Report(c)
    r = gr.run_sh(gr.OracleBackend(oracle_mod), c, rep, free)
    rep.finish()
    if not free:
        gr.assert_sh_clamp_populated(c, r)


# ------------------------------------------------------------------ dynamic evaluation
def _gold(name):
    return dict(np.load(os.path.join(HERE, "golden", name)))


def test_dynamic_twin_matches_reference_vectors():
    """the float64 twin of the dynamic evaluation against the reference's own float32 results (dynamic_400x50.npz), at the
    tolerances tests/test_dynamic_cpu.py holds the C oracle to; both table layouts of the twin agree exactly"""
    from splatter_a_video_amd.dynamics import FrameClock
    g = _gold("dynamic_400x50.npz")
    N, T, I = g["position"].shape[0], int(g["T"]), int(g["I"])
    c = dict(N=N, T=T, I=I, clock=FrameClock(T, g["intervals"], int(g["start_frame_id"]), int(g["time_len"])),
             position=g["position"], cubic=g["pos_cubic_node"], rotation=g["rotation"], rot_poly=g["rot_poly_feat"],
             rot_fourier=g["rot_fourier_feat"], opacity=g["opacity"], scaling=g["scaling"])
    for t in g["times"]:
        pre = f"t{t}_"
        c.update(g_pos=g[pre + "g_pos"], g_rot=g[pre + "g_rot"], g_opa=g[pre + "g_opa"], g_scl=g[pre + "g_scl"])
        r = gr.dyn_ref(c, int(t))
        np.testing.assert_allclose(r["pos"], g[pre + "pos"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(r["rot"], g[pre + "rot"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(r["opa"], g[pre + "opa"], rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(r["scl"], g[pre + "scl"], rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(r["d_position"], g[pre + "d_position"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(r["d_cubic"], g[pre + "d_cubic"], rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(r["d_rotation"], g[pre + "d_rotation"], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(r["d_opacity"], g[pre + "d_opacity"], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(r["d_scaling"], g[pre + "d_scaling"], rtol=2e-6, atol=1e-9)
        r2 = gr.dyn_ref(c, int(t), tw.SEGMENT_MAJOR)
        assert torch.equal(r2["pos"], r["pos"]) and torch.equal(r2["d_cubic"], r["d_cubic"])


def test_poly_fourier_twin_matches_reference_vectors():
    from splatter_a_video_amd.dynamics import FrameClock
    g = _gold("polyfourier_300x40.npz")
    T = int(g["time_len"]) + 1
    c = dict(N=g["position"].shape[0], T=T, clock=FrameClock(T, None, int(g["start_frame_id"]), int(g["time_len"])),
             position=g["position"], pos_poly=g["pos_poly_feat"], pos_fourier=g["pos_fourier_feat"])
    for t in g["times"]:
        c["g_pos"] = g[f"t{t}_g_pos"]
        r = gr.ppf_ref(c, int(t))
        np.testing.assert_allclose(r["pos"], g[f"t{t}_pos"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(r["d_position"], g[f"t{t}_d_position"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(r["d_poly"], g[f"t{t}_d_pos_poly"], rtol=2e-6, atol=1e-6)
        np.testing.assert_allclose(r["d_fourier"], g[f"t{t}_d_pos_fourier"], rtol=2e-6, atol=1e-6)


@pytest.mark.parametrize("N", gr.DYN_SIZES)
def test_oracle_dynamics_meet_the_bars(oracle_mod, N):
    c = gr.make_dyn_case(N)
    rep = gr.Report(c)
    for t in c["times"]:
        gr.run_dyn(gr.OracleBackend(oracle_mod), c, rep, t)
        gr.run_ppf(gr.OracleBackend(oracle_mod), c, rep, t)
    rep.finish()


@pytest.mark.parametrize("cid", ["o257", "o100003"])
def test_oracle_frame_preprocess_meets_the_bars(oracle_mod, cid):
    """dynamic evaluation followed by the orthographic chain (what dynamics.frame_preprocess fuses)"""
    c = gr.make_dyn_geom_case(cid)
    rep = gr.Report(c)
    for t in (0, c["times"][2], c["T"] - 1):
        r, masks = gr.run_frame_preprocess(gr.OracleBackend(oracle_mod), c, rep, t, tw.GAUSSIAN_MAJOR)
        gr.assert_caps(c, masks)
        assert gr.conditioned_share(r) >= 0.95
    rep.finish()


# ------------------------------------------------------------------ the constants and the twin itself
def test_constants_come_from_the_committed_measurement():
    """the slope of the conditioning rule is 4 x the envelope the float32 C oracle measured on these cases
    (tools/geometry_reference_report.py --backend oracle), and the record was taken with the constants in force"""
    with open(os.path.join(HERE, "..", "profiles", "geometry_reference_cpu_float32.json")) as f:
        rec = json.load(f)
    assert rec["backend"] == "oracle"
    assert gr.WIDEN_SLOPE == rec["widen_slope_from_envelope"] == max(1.0, round(4.0 * rec["envelope_max"] + 0.005, 2))
    for k, v in rec["constants"].items():
        assert getattr(gr, k) == v, k
    assert max(v for d in rec["worst"].values() for s, v in d.items() if s != "all") <= 1.0
    assert min(rec["live_share_below_KAPPA0"].values()) >= 0.95


def test_extended_twin_gradcheck():
    """autograd of the twin's new differentiable outputs against finite differences (float64, a few generic rows)"""
    torch.manual_seed(0)
    n = 4
    f64 = lambda *s: torch.randn(*s, dtype=torch.float64)
    for ortho in (False, True):
        c = gr.case_by_id("o257" if ortho else "p257")
        rows = slice(c["n_edge"], c["n_edge"] + n)
        xyz = gr.T64(c["xyz"][rows]).requires_grad_(True)
        intr, extr = gr.T64(c["intr"]).requires_grad_(True), gr.T64(c["extr"][:3, :4]).requires_grad_(True)
        cov = tw.cov3d(gr.T64(c["scale"][rows]) * 30, gr.T64(c["quat"][rows])).requires_grad_(True)
        uv = tw.project_full(xyz, intr, extr, c["W"], c["H"], 0.0, 0.0, ortho)["uv"].detach()

        def proj(x, i, e):
            p = tw.project_full(x, i, e, c["W"], c["H"], 0.0, 0.0, ortho)
            return p["uv"], p["depth"]

        def conic(x, cv, i, e):
            return tw.ewa_full(x, cv, i, e, uv, c["W"], c["H"], torch.ones(n), ortho)["conic"]

        assert torch.autograd.gradcheck(proj, (xyz, intr, extr), eps=1e-6, atol=1e-5, rtol=1e-4)
        assert torch.autograd.gradcheck(conic, (xyz, cov, intr, extr), eps=1e-6, atol=1e-5, rtol=1e-4)
    for deg in range(4):
        sh, d = f64(n, (deg + 1) ** 2, 3).requires_grad_(True), f64(n, 3).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda a, b: tw.sh_full(a, deg, b, torch.ones(n), True)["color"], (sh, d))
    I, basis = 3, f64(12)
    pos, cub = f64(n, 3).requires_grad_(True), f64(n, 4 * I * 3).requires_grad_(True)
    for layout in (tw.GAUSSIAN_MAJOR, tw.SEGMENT_MAJOR):
        assert torch.autograd.gradcheck(lambda p, t: tw.dyn_position(p, t, 1, 0.37, I, layout), (pos, cub))
    rot, rp, rf = f64(n, 4).requires_grad_(True), f64(n, 4, 4) * 0.05, f64(n, 8, 4) * 0.05
    assert torch.autograd.gradcheck(lambda r: tw.dyn_rotation(r, rp, rf, basis), (rot,))
    pp, pf = f64(n, 4, 3).requires_grad_(True), f64(n, 8, 3).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda p, a, b: tw.position_poly_fourier(p, a, b, basis), (pos, pp, pf))


@pytest.mark.parametrize("cid", ["o257", "p257", "o3001", "p3001"])
def test_batch_frame_cameras_keep_the_caps(cid):
    """the per-frame cameras and offsets the FrameBatch test renders with leave no more rows out than the caps allow"""
    c = gr.case_by_id(cid)
    for fc in gr.frame_cases(c, 3, offsets=not c["ortho"]):
        r = gr.chain_ref(fc, offset=not c["ortho"])
        d, _ = gr.ewa_rows(r, r["mag_u"], r["mag_v"], r["cull_safe"])
        gr.assert_caps(fc, dict(det=~d["dead"], ceil=d["ceil_safe"], floor=d["floor_safe"]))
        assert gr.conditioned_share(r) >= 0.95
