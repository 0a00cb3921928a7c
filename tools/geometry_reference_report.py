"""Worst error of the per-Gaussian geometry against the float64 twin, as a fraction of its bar, per quantity and stratum.

    python tools/geometry_reference_report.py --backend oracle --out profiles/geometry_reference_cpu_float32.json
    python tools/geometry_reference_report.py --backend hip    --out profiles/geometry_reference_gpu.json

Reuses the cases, bars and margins of tests/geometry_ref.py (nothing is asserted here).  ``--backend oracle`` is the float32
C oracle on the CPU: its record also holds the envelope of the ill-conditioned rows (error as a fraction of the PLAIN bar
per unit of kappa / KAPPA0) from which geometry_ref.WIDEN_SLOPE = 4 x envelope is taken, the rows each decision leaves
out, and the share of live rows below the conditioning threshold.
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import geometry_ref as gr   # noqa: E402
import torch_twin as tw     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["oracle", "hip"], required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.backend == "oracle":
        import oracle
        oracle.build(); oracle.set_threads(1)
        backend, layouts = gr.OracleBackend(oracle), [tw.GAUSSIAN_MAJOR]
    else:
        import torch
        backend, layouts = gr.HipBackend(torch.device("cuda:0")), [tw.GAUSSIAN_MAJOR, tw.SEGMENT_MAJOR]
    worst, envelope, excluded, share = {}, {}, {}, {}

    def take(rep, masks=None, e=None, key=None):
        for (q, s), v in rep.worst.items():
            worst.setdefault(q, {})
            worst[q][s] = max(worst[q].get(s, 0.0), v)
        for q, v in rep.envelope.items():
            envelope[q] = max(envelope.get(q, 0.0), v)
        if masks is not None:
            excluded[key] = {k: list(v) for k, v in gr.exclusion_counts(rep.case, masks).items()}
        if e is not None:
            share[key] = gr.conditioned_share(e)

    for cid in gr.CASE_IDS:
        c = gr.case_by_id(cid)
        rep = gr.Report(c)
        _, e, masks = gr.run_operators(backend, c, rep)
        take(rep, masks, e, cid + ".operators")
        for offset in (False, True):
            rep = gr.Report(c)
            r, masks = gr.run_fused(backend, c, rep, offset)
            take(rep, masks, r, f"{cid}.fused.offset{int(offset)}")
    for deg in range(4):
        for free in (False, True):
            c = gr.make_sh_case(deg)
            rep = gr.Report(c)
            gr.run_sh(backend, c, rep, free)
            take(rep)
    for N in gr.DYN_SIZES:
        c = gr.make_dyn_case(N)
        rep = gr.Report(c)
        for t in c["times"]:
            for layout in layouts:
                gr.run_dyn(backend, c, rep, t, layout)
            gr.run_ppf(backend, c, rep, t)
        take(rep)
    for cid in ("o257", "o100003"):
        c = gr.make_dyn_geom_case(cid)
        for t in (0, c["times"][2], c["T"] - 1):
            for layout in layouts:
                rep = gr.Report(c)
                r, masks = gr.run_frame_preprocess(backend, c, rep, t, layout)
                take(rep, masks, r, f"{c['id']}.t{t}.layout{layout}")
    env = max(envelope.values()) if envelope else 0.0
    out = dict(backend=a.backend, what="worst |error| / bar per quantity and stratum (1.0 = on the bar); counts for the integer outputs",
               constants=dict(KAPPA0=gr.KAPPA0, WIDEN_SLOPE=gr.WIDEN_SLOPE, KAPPA_DEAD=gr.KAPPA_DEAD, CULL_MULT=gr.CULL_MULT,
                              RADIUS_MULT=gr.RADIUS_MULT, FLOOR_MULT=gr.FLOOR_MULT, SH_MULT=gr.SH_MULT, EXCLUDE_CAP=gr.EXCLUDE_CAP),
               worst={q: {s: float(f"{v:.4g}") for s, v in d.items()} for q, d in sorted(worst.items())},
               envelope_per_quantity={q: float(f"{v:.4g}") for q, v in sorted(envelope.items())},
               envelope_max=float(f"{env:.4g}"), widen_slope_from_envelope=max(1.0, round(4.0 * env + 0.005, 2)))
    if a.backend == "oracle":
        out.update(rows_left_out_bulk_and_deliberate=excluded, live_share_below_KAPPA0=share)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(envelope_max=out["envelope_max"], slope=out["widen_slope_from_envelope"],
                          worst_overall=max(v for d in worst.values() for s, v in d.items() if s != "all"))))


if __name__ == "__main__":
    main()
