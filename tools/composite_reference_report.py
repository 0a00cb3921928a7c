"""Worst error of the compositing kernels against the float64 reference of tests/composite_ref.py, as a fraction of the bar.

    python tools/composite_reference_report.py --backend float32 --out profiles/composite_reference_cpu_float32.json
    python tools/composite_reference_report.py --backend hip     --out profiles/composite_reference_gpu.json
    python tools/composite_reference_report.py --backend hip-frames --out profiles/frames_composite_reference_gpu.json
    python tools/composite_reference_report.py --backend float32-points --out profiles/points_reference_cpu_float32.json
    python tools/composite_reference_report.py --backend hip-points --out profiles/points_composite_reference_gpu.json

``--backend float32`` is the numpy float32 restatement of the kernels' arithmetic on the CPU: its worst error / companion per
output gives the K of every bar (smallest power of two at or above 4 x the ratio), which tests/test_composite_ref_cpu.py
re-checks.  ``--backend hip`` runs every case of tests/test_gpu_composite_reference.py and records the worst error / bar per
route and output, what the kernels write into the gradient rows of non-finite operands, and the library's build id.
``--backend hip-frames`` does the same for the frame batch's entry points (tests/test_gpu_frames_composite_reference.py).
``--backend float32-points`` is the float32 restatement of the sparse compositing kernels (tests/points_ref.py f32_points): its
ratios decide whether a sparse output reuses the dense K or gets one of its own (tests/test_points_ref_cpu.py re-checks);
``--backend hip-points`` runs every case of tests/test_gpu_points_reference.py (csrc/query.hip against the float64 points
reference).
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["float32", "hip", "hip-frames", "float32-points", "hip-points"], required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import oracle
    oracle.build()
    oracle.set_threads(1)
    if a.backend == "float32":
        import test_composite_ref_cpu as t
        rec = t.record(oracle)
    elif a.backend == "float32-points":
        import test_points_ref_cpu as t
        rec = t.record(oracle)
    else:
        import torch
        from splatter_a_video_amd import _lib as L
        if a.backend == "hip-frames":
            import test_gpu_frames_composite_reference as t
        elif a.backend == "hip-points":
            import test_gpu_points_reference as t
        else:
            import test_gpu_composite_reference as t
        worst, nonfinite = t.measure()
        rnd = lambda d: {k: (rnd(v) if isinstance(v, dict) else float(f"{v:.4g}")) for k, v in sorted(d.items())}
        rec = dict(what="worst |error| / bar per route and output (1.0 = on the bar; bar = K x companion, K from "
                        "composite_reference_cpu_float32.json, for hip-points as points_reference_cpu_float32.json resolves it); integer outputs are compared exactly and carry no figure",
                   backend="hip", build_id=L.build_id(), device=torch.cuda.get_device_name(0), K=t.K_BAR, worst=rnd(worst),
                   nonfinite_rows_written=nonfinite)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec.get("worst", rec.get("K"))))


if __name__ == "__main__":
    main()
