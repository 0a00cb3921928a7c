"""The reference's layer edits restated in numpy on top of the CPU oracle's dynamic evaluation (test infrastructure).

``render_part`` (reference src/trainer_fragGS.py:1310-1341) keeps the rows of the evaluated model that a mask selects (:1323);
``add_fg`` (:1344-1405) concatenates, behind the whole model at the frame's time (:1350), the selected rows of the model
evaluated at a second time (:1356): their positions scaled about their own mean and shifted (:1359-1362), their rotations
(:1365-1371: a quaternion -> matrix -> quaternion round trip that returns +-q, not restated: q is used) and every other
attribute unchanged (:1384-1387).  A scene here is a list of layers -- dicts ``select`` (bool [N] or None), ``times`` (one per
clip frame, or None: the clip's), ``scale``, ``delta`` (None, [3] or [T, 3]), ``scale_splats`` -- and a frame's arrays are the
layers' rows concatenated in order, every array float32, the transform in the reference's order with every step rounded to
float32 and the centroid ``float32(mean in float64)``."""
import numpy as np


def transformed(layer) -> bool:
    return float(layer.get("scale", 1.0)) != 1.0 or layer.get("delta") is not None


def evaluate(o, clock, host, t):
    seg, d, basis = clock.scalars(t)
    b = np.array(list(basis), np.float32)
    return o.dynamic_eval_forward(host["position"], host["pos_cubic_node"], host["rotation"], host["rot_poly_feat"],
                                  host["rot_fourier_feat"], host["opacity"], host["scaling"], seg, d, b[:4], b[4:])


def place(pos, scale, delta):
    """(:1359-1362) ``pos`` float32 [S, 3] -> ((pos - mean) * scale + mean) + delta, float32 at every step"""
    c = pos.astype(np.float64).mean(axis=0, keepdims=True).astype(np.float32)
    out = ((pos - c) * np.float32(scale)).astype(np.float32)
    out = (out + c).astype(np.float32)
    if delta is not None:
        out = (out + np.asarray(delta, np.float32).reshape(1, 3)).astype(np.float32)
    return out, c


def frame_arrays(o, clock, host, layers, times, f, features=()):
    """arrays of clip frame ``f``: dict position [Q,3], rotation [Q,4], scale [Q,3], opacity [Q,1], features (list of [Q,c]),
    centroids (per layer, None for an untransformed one)"""
    N = host["position"].shape[0]
    pos_l, rot_l, scl_l, opa_l, cen_l = [], [], [], [], []
    feat_l = [[] for _ in features]
    for layer in layers:
        t = times[f] if layer.get("times") is None else layer["times"][f]
        pos, rot, opa, scl = evaluate(o, clock, host, t)
        sel = np.ones(N, bool) if layer.get("select") is None else np.asarray(layer["select"], bool)
        pos, rot, opa, scl = pos[sel], rot[sel], opa[sel], scl[sel]
        cen = None
        if transformed(layer):
            delta = layer.get("delta")
            if delta is not None:
                delta = np.asarray(delta, np.float32)
                delta = delta if delta.ndim == 1 else delta[f]
            s = float(layer.get("scale", 1.0))
            pos, cen = place(pos, s, delta)
            if layer.get("scale_splats"):
                scl = (scl * np.float32(s)).astype(np.float32)
        pos_l.append(pos); rot_l.append(rot); scl_l.append(scl); opa_l.append(opa); cen_l.append(cen)
        for k, ft in enumerate(features):
            feat_l[k].append(np.asarray(ft, np.float32)[sel])
    cat = lambda xs: np.ascontiguousarray(np.concatenate(xs, 0), dtype=np.float32)
    return dict(position=cat(pos_l), rotation=cat(rot_l), scale=cat(scl_l), opacity=cat(opa_l),
                features=[cat(x) for x in feat_l], centroids=cen_l)
