"""Worst error of the frame batch's Gaussian-side backward against float64, as a fraction of its bar, per case and output.

    python tools/gauss_backward_reference_report.py --backend oracle --out profiles/gauss_backward_reference_cpu_float32.json
    python tools/gauss_backward_reference_report.py --backend hip    --out profiles/gauss_backward_reference_gpu.json

Reuses the problems, references and bars of tests/gauss_backward_ref.py (nothing is asserted here).  ``--backend oracle`` is
the float32 C oracle's operator chain on the CPU, ``--backend hip`` the kernels as tests/test_gpu_gauss_backward_reference.py
calls them.
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gauss_backward_ref as gb   # noqa: E402
import geometry_ref as gr         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["oracle", "hip"], required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    reports = []
    if a.backend == "oracle":
        import oracle
        oracle.build(); oracle.set_threads(1)
        for lkey in ("plain_narrow", "sets_wide"):
            for F in gb.CHAIN_F:
                for cam in sorted(gb.CHAIN_CAMS):
                    P = gb.static_problem(F, cam, lkey)
                    rep = gr.Report(P["c"])
                    gb.check_chain(rep, "", gb.oracle_static(oracle, P["frames"], P["R"], P["S"], P["depth_channel"]), P["ref"])
                    reports.append(rep)
            for name in sorted(gb.DYN_TIMES):
                P = gb.dyn_problem(name, lkey)
                rep = gr.Report(P["c"])
                gb.check_chain(rep, "", gb.oracle_dynamic(oracle, gb.dyn_case(), P["times"], P["R"], P["S"], P["depth_channel"]),
                               P["ref"])
                reports.append(rep)
    else:
        import torch
        import test_gpu_gauss_backward_reference as t
        dev = torch.device("cuda:0")
        for lkey in gb.CHAIN_LAYOUTS:
            for F in gb.CHAIN_F:
                for cam in sorted(gb.CHAIN_CAMS):
                    reports.append(t.run_static_chain(dev, F, cam, lkey))
            for name in sorted(gb.DYN_TIMES):
                reports.append(t.run_dyn_chain(dev, name, lkey))
    out = gb.report_json(a.out, a.backend, reports)
    print(json.dumps(dict(worst_overall=out["worst_overall"], failures=sum(len(r.fail) for r in reports))))
    for r in reports:
        for line in r.fail:
            print(r.case["id"], line[:300])


if __name__ == "__main__":
    main()
