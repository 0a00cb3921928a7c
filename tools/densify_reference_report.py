"""Worst error of the densification kernels against the references of tests/densify_ref.py, as a fraction of the bar.

    python tools/densify_reference_report.py --backend float32 --out profiles/densify_reference_cpu_float32.json
    python tools/densify_reference_report.py --backend hip     --out profiles/densify_reference_gpu.json

``--backend float32`` is the numpy float32 restatement of the kernels' arithmetic on the CPU (the envelope
tests/test_densify_ref_cpu.py re-checks), ``--backend hip`` the kernels as tests/test_gpu_densify_reference.py and
tests/test_gpu_train_step_densify.py call them.
The bars come from the derivations in tests/densify_ref.py, not from these files.
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import densify_ref as dr   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["float32", "hip"], required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rnd = lambda d: {k: (rnd(v) if isinstance(v, dict) else float(f"{v:.4g}")) for k, v in sorted(d.items())}
    rec = {"constants": dict(K_POS=dr.K_POS, K_SCL=dr.K_SCL, K_BM=dr.K_BM, MULT=dr.MULT, EXCLUDE_CAP=dr.EXCLUDE_CAP),
           "what": "worst |error| / bar (1.0 = on the bar); decisions: share of rows left out of a comparison and rows that differ"}
    if a.backend == "float32":
        import test_densify_ref_cpu as t
        rec.update(backend="numpy_float32", envelope=rnd(t.envelope()))
        rec["excluded_share"] = rnd({dr.mask_case(N, p)["id"]: {k: dr.excluded_share(dr.mask_case(N, p), k) for k in ("clone", "split", "prune")}
                                     for N in dr.MASK_N for p in dr.MASK_PARAMS})
    else:
        import torch
        from splatter_a_video_amd import _lib as L
        import test_gpu_densify_reference as t
        import test_gpu_train_step_densify as ts
        worst = t.measure()
        worst["train_step_children"] = {mode: ts.run(mode) for mode in sorted(ts.MODES)}
        rec.update(backend="hip", build_id=L.build_id(), device=torch.cuda.get_device_name(0), worst=rnd(worst))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec.get("envelope", rec.get("worst"))))


if __name__ == "__main__":
    main()
