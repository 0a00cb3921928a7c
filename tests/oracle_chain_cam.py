"""tests/oracle_chain.py's dynamic_frames with a camera PER FRAME and / or the pinhole camera (test infrastructure): frame f is
the oracle's dynamic evaluation, its static chain (oracle_chain.frame) under frame f's camera with frame f's slices of the
image gradients, and its dynamic backward; the parameter gradients are summed over the frames -- what one backward of the
batch gives.  Used by tests/test_gpu_views_backward.py."""
import numpy as np

import oracle_chain as oc


def dynamic_frames_cam(o, clock, times, host, extr, intr, W, H, sets, grads, K=0, nearest=0.01):
    """``extr`` [4,4] or [F,4,4]; ``intr`` None (orthographic), [4] or [F,4].  Returns (per-frame results of oracle_chain.frame,
    totals: position, pos_cubic_node [N,4,I,3], rotation, opacity, scaling, feats (per set, None for depth), tap, abs_tap)."""
    N = host["position"].shape[0]
    I = clock.interval_num
    tot = dict(position=0.0, pos_cubic_node=0.0, rotation=0.0, opacity=0.0, scaling=0.0, feats=None, tap=0.0, abs_tap=0.0)
    per = []
    for f, t in enumerate(times):
        seg, d, basis = clock.scalars(t)
        b = np.array(list(basis), np.float32)
        pos, rot, opa, scl = o.dynamic_eval_forward(host["position"], host["pos_cubic_node"], host["rotation"],
                                                    host["rot_poly_feat"], host["rot_fourier_feat"], host["opacity"],
                                                    host["scaling"], seg, d, b[:4], b[4:])
        e = extr[f] if np.ndim(extr) == 3 else extr
        k = None if intr is None else (intr[f] if np.ndim(intr) == 2 else intr)
        r = oc.frame(o, pos, scl, rot, opa, e, W, H, sets, [g[f] for g in grads], K, nearest=nearest, intr=k)
        per.append(r)
        g = r["d"]
        dpos, dcub, drot, dopa, dscl = o.dynamic_eval_backward(
            (N, 4, I, 3), host["rotation"], host["rot_poly_feat"], host["rot_fourier_feat"], host["opacity"], host["scaling"],
            seg, d, b[:4], b[4:], g["xyz"].astype(np.float32), g["rotate"].astype(np.float32), g["opacity"].astype(np.float32),
            g["scale"].astype(np.float32))
        for name, v in (("position", dpos), ("pos_cubic_node", dcub), ("rotation", drot), ("opacity", dopa), ("scaling", dscl)):
            tot[name] = tot[name] + v.astype(np.float64)
        tot["feats"] = g["feats"] if tot["feats"] is None else [None if a is None else a + c for a, c in zip(tot["feats"], g["feats"])]
        if g["tap"] is not None:
            tot["tap"] = tot["tap"] + g["tap"]
            tot["abs_tap"] = tot["abs_tap"] + g["abs_tap"]
    return per, tot
