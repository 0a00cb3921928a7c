"""The camera gradients of a dynamic frame batch (splat_frames_camera_backward_dynamic, include/splat_hip_camera_grad.h) in
float64: per frame the chain of geometry_ref.chain_ref -- tw.dyn_position / dyn_rotation / dyn_scaling -> tw.project_full ->
tw.cov3d -> tw.ewa_full -- with ``intr`` and ``extr[:3, :4]`` as the leaves and the frame's summed pair records
(gauss_backward_ref.upstream) as the upstream gradients.  Shared by tests/test_camera_grad_ref_cpu.py (float32 attains the bar)
and the GPU tests.  No GPU call at import.

The chain runs over the rows that OWN RECORDS in the frame and over no other: a row without records contributes exactly
nothing.  The cases hold rows with non-finite positions (the "edge" stratum); a chain over all rows multiplies their
coordinates by a zero upstream gradient and returns NaN (tests/test_camera_grad_ref_cpu.py records it for "ortho_pf").

Problems: those of tests/gauss_backward_cam_ref.py ("ortho_pf", "pinhole_pf" over TIMES, "pinhole_one" over ONE_TIMES) in the
record layouts "plain_narrow" (no depth column) and "sets_wide" (depth column 12 + 3), and "ortho_one": the orthographic case
under its ONE camera (stride 0 for an orthographic camera).

Bar: geometry_ref.Report.tensor, the project's rule for sums over rows -- 2e-3 |b| + 1e-4 max|b| per frame and tensor ([3,4]
and [4]); for a shared camera over the frame-summed tensor.  Onto a pre-fill v: + 2^-24 |v + b|, the one float32 addition
(gauss_backward_ref.check_chain's rule).  No outlier budget.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

import gauss_backward_cam_ref as gc
import gauss_backward_ref as gb
import geometry_ref as gr
import torch_twin as tw

MODES = dict(gc.MODES, ortho_one=dict(cid="o257", ortho=True, per_frame=False, cam=0))
LAYOUTS = ("plain_narrow", "sets_wide")
SIZES = (1, 63, 65, 257)
PARAMS = ("position", "cubic", "rotation", "rot_poly", "rot_fourier", "opacity", "scaling", "g_pos", "g_rot", "g_opa", "g_scl")


def problems():
    return gc.problems() + [("ortho_one", n) for n in gc.ONE_TIMES]


def dyn_case(mode):
    return gb.dyn_case() if mode == "ortho_one" else gc.dyn_case(mode)


def frame_camera(mode, c, f):
    return (c["intr"], c["extr"]) if mode == "ortho_one" else gc.frame_camera(mode, c, f)


def eligibility(mode, name):
    return gb.dyn_eligibility(name) if mode == "ortho_one" else gc.eligibility(mode, name)


def subcase(c, idx):
    """the case restricted to the rows ``idx``"""
    return dict(c, N=len(idx), stratum=c["stratum"][idx], **{k: c[k][idx] for k in PARAMS})


def frame_grads(c, intr, extr, t, up, idx, dtype=torch.float64, decide=True):
    """(dL/dintr [4], dL/dextr [3,4]) of frame time ``t`` under (intr, extr) over the rows ``idx`` of the case; ``up``: the
    upstream gradients of ALL rows (gauss_backward_ref.upstream).  ``decide=False``: the rows are taken as visible with a
    radius, without the float64 cull / tile-rectangle decisions (records of a real forward: the library has decided in
    float32, and the kernel differentiates through no decision)"""
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    K, E = T(intr).requires_grad_(True), T(extr[:3, :4]).requires_grad_(True)
    if len(idx) == 0:
        return torch.zeros(4, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.float64)
    seg, d, basis = gr._basis64(c["clock"], t)
    n, I = len(idx), c["I"]
    x = tw.dyn_position(T(c["position"][idx]), T(c["cubic"][idx]).reshape(n, 4, I, 3), seg, d, I, tw.GAUSSIAN_MAJOR)
    q = tw.dyn_rotation(T(c["rotation"][idx]), T(c["rot_poly"][idx]), T(c["rot_fourier"][idx]), basis.to(dtype))
    s = tw.dyn_scaling(T(c["scaling"][idx]))
    p = tw.project_full(x, K, E, c["W"], c["H"], c["nearest"], c["extent"], c["ortho"])
    if decide:
        vis = ~p["cull"]
        e = tw.ewa_full(x, tw.cov3d(s, q, vis), K, E, p["uv"], c["W"], c["H"], vis, c["ortho"])
    else:
        depth = tw.cam_xform(x, E)[:, 2:3]
        p = dict(uv=torch.stack([p["u"], p["v"]], -1), depth=depth)
        e = dict(conic=tw.ewa(x, tw.cov3d(s, q), K, E, c["W"], c["H"], torch.ones(n, dtype=torch.bool), c["ortho"]))
    g_uv, g_d, g_c = T(up["g_uv"][idx]), T(up["g_d"][idx]), T(up["g_conic"][idx])
    loss = (torch.nan_to_num(p["uv"]) * g_uv).sum() + (torch.nan_to_num(p["depth"]) * g_d).sum() + (e["conic"] * g_c).sum()
    dK, dE = torch.autograd.grad(loss, [K, E], allow_unused=True)
    dK = torch.zeros_like(K) if dK is None else dK
    return dK.double(), dE.double()


def reference(mode, c, times, R, S, depth_channel, dtype=torch.float64, masked=True):
    """dict(intr [F,4], extr [F,3,4]) float64: frame f's sums under frame f's camera; ``masked=False``: the chain over ALL
    rows (what the kernel must not compute)"""
    P = R["P"]
    di, de = [], []
    for f, t in enumerate(times):
        intr, extr = frame_camera(mode, c, f)
        idx = np.nonzero(R["cnt"][f] > 0)[0] if masked else np.arange(P)
        a, b = frame_grads(c, intr, extr, t, gb.upstream(R, S, f, depth_channel), idx, dtype)
        di.append(a); de.append(b)
    return dict(intr=torch.stack(di), extr=torch.stack(de))


def layout_of(lkey):
    lay, dch = gb.chain_layout(lkey)
    return lay, (dch if lay["kind"] == "sets" else -1)


@functools.lru_cache(maxsize=None)
def problem(mode, name, lkey, P=None):
    """records over the first ``P`` rows of the mode's case (default: all 257) and their float64 camera gradients"""
    c = dyn_case(mode)
    P = c["N"] if P is None else P
    times = gb.DYN_TIMES[name]
    lay, dch = layout_of(lkey)
    elig = eligibility(mode, name)[:, :P]
    R = gb.build_records(gb.count_table(len(times), P) * elig, lay, seed=len(times) + 90 + MODES[mode]["cam"] + P)
    S = gb.segment_sums(R)
    case = dict(c, id=f"camgrad.{mode}.{name}.{lkey}.P{P}")
    return dict(c=case, mode=mode, times=times, R=R, S=S, depth_channel=dch, P=P, ref=reference(mode, c, times, R, S, dch))


def shared(mode):
    return not MODES[mode]["per_frame"]


def check(rep, tag, got_extr, got_intr, ref, share, pre_extr=None, pre_intr=None):
    """the outputs ([F,12] / [F,4], or one row for a shared camera) against ``ref`` at the bar"""
    def one(name, got, b, pre):
        got = gr.T64(np.asarray(got, np.float64)).reshape(b.shape)
        if pre is None:
            rep.tensor(name, got, b)
            return
        v = gr.T64(np.asarray(pre, np.float64)).reshape(b.shape)
        bar = 2e-3 * b.abs() + 1e-4 * b.abs().max() + gr.EPS32 * (v + b).abs()
        w = float(((got - (v + b)).abs() / torch.clamp_min(bar, 1e-300)).max())
        rep.worst[(name, "all")] = max(rep.worst.get((name, "all"), 0.0), w)
        if not w <= 1:
            rep.fail.append(f"{name}: {w:.3g}x the bar, got {got.tolist()} want {(v + b).tolist()}")
    for key, got, pre in (("extr", got_extr, pre_extr), ("intr", got_intr, pre_intr)):
        if got is None:
            continue
        b = ref[key]
        if share:
            one(f"{tag}dL_d{key}", got, b.sum(0), pre)
        else:
            got = np.asarray(got).reshape(b.shape[0], -1)
            for f in range(b.shape[0]):
                one(f"{tag}dL_d{key}[{f}]", got[f], b[f], None if pre is None else np.asarray(pre).reshape(b.shape[0], -1)[f])


# ------------------------------------------------------------------ device side
def dyn_geometry(mode, c, times, layout, device, P=None):
    if mode != "ortho_one":
        return gc.dyn_geometry(mode, c, times, layout, device, P)
    g = gb.dyn_geometry(c, times, layout, device, P)
    g["intr"] = None
    g["cam"] = gb.camera_struct(g["extr"])
    return g


def partials(F, P, device):
    L = gb.lib()
    return torch.empty(int(L.lib().splat_camera_grad_partials_floats(F, P)), dtype=torch.float32, device=device)


def call_camera_backward(D, g, W, H, depth_column, part, d_extr, d_intr, cam=None):
    L = gb.lib()
    L.check(L.lib().splat_frames_camera_backward_dynamic(
        D["F"], D["P"], g["I"], W, H, D["cap"], D["layout"]["stride"], depth_column, L.ptr(D["d_rec"]), L.ptr(D["d_goff"]),
        L.ptr(g["tab"]), L.ptr(g["position"]), L.ptr(g["cubic"]), g["layout"], L.ptr(g["rotation"]), L.ptr(g["rot_poly"]),
        L.ptr(g["rot_fourier"]), L.ptr(g["scaling"]), ctypes.byref(g["cam"] if cam is None else cam), L.ptr(part),
        L.ptr(d_extr), L.ptr(d_intr), L.stream()))
    gb._sync()


def depth_column(R, depth_channel):
    return R["layout"]["ng"] + depth_channel if depth_channel >= 0 else -1
