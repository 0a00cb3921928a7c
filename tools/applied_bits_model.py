"""CPU model of what the narrow backward's quarter lists lose when they are built from the (entry, quarter) pairs that APPLIED
in the forward instead of the pairs its geometric cull could not exclude.  Tools only; imports the oracle for the
geometry and the tile lists of the bench scene (300k Gaussians, 854 x 480).

  1. per (tile, splat) pair of a sample of Gaussians: 4x4 quarters kept by the cull's rule for rows below 16 channels (bounding box,
     then the tangent-plane bound -- tools/cull_model.py) and quarters with at least one pixel centre inside the alpha >= 1/255
     ellipse;
  2. on a sample of tiles, with the depth-sorted list walked in float64 under the reference's rules (saturation included): the
     backward's steps, sum of ceil(list length / 16) over the quarter lists of its 128-entry super-batches (cut from the back of
     the entries below the tile's largest ncontrib), for both kinds of words -- every list on its own, and with the four waves
     of a tile coupled by the barrier of a super-batch (the longest wave counts) -- and the fill of the steps.

usage: python tools/applied_bits_model.py [gaussians sampled] [tiles sampled]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import oracle
from splatter_a_video_amd.synth import make_scene

N, W, H, SB = 300000, 854, 480, 128
NG = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
NT = int(sys.argv[2]) if len(sys.argv) > 2 else 120
sc = make_scene(N, W, H, seed=1234)
xyz = sc.positions(0)
uv, depth = oracle.project_point_ortho_forward(xyz, sc.extr, W, H, nearest=0.01)
cov = oracle.compute_cov3d_forward(sc.scale, sc.rotate)
conic, radius, tiles = oracle.ewa_project_forward(xyz, cov, sc.intr, sc.extr, uv, W, H, visible=None, ortho=True)
uv, conic, op = uv.astype(np.float64), conic.astype(np.float64), sc.opacity.astype(np.float64).reshape(-1)
gx, gy = (W + 15) // 16, (H + 15) // 16
PX, PY = np.meshgrid(np.arange(16), np.arange(16))
QOF = ((PX >> 2) + 4 * (PY >> 2)).reshape(-1)                       # pixel -> quarter 0 .. 15 of the tile (4 x 4 quarters)
ONEHOT = (QOF[:, None] == np.arange(16)[None, :]).astype(np.float64)
WAVE_OF_Q = np.array([(q % 4) // 2 + 2 * ((q // 4) // 2) for q in range(16)])


def rule_quarters(ids, tx0, ty0):
    """[L, 16] quarters the cull's rule keeps (bounding box + tangent plane), float64, without its rounding allowances"""
    u, v, A, B, C, o = uv[ids, 0], uv[ids, 1], conic[ids, 0], conic[ids, 1], conic[ids, 2], op[ids]
    live = 255.0 * o >= 0.999
    tau = 2.0 * np.log(np.maximum(255.0 * o, 1.0))
    det = A * C - B * B
    hx, hy = np.sqrt(tau * C / det), np.sqrt(tau * A / det)
    keep = np.zeros((len(ids), 16), bool)
    for q in range(16):
        x0, y0 = tx0 + 4 * (q % 4), ty0 + 4 * (q // 4)
        ax = np.maximum(np.maximum(x0 - u, u - (x0 + 3.0)), 0.0)
        ay = np.maximum(np.maximum(y0 - v, v - (y0 + 3.0)), 0.0)
        cx, cy = x0 + 1.5 - u, y0 + 1.5 - v
        t1, t2 = A * cx + B * cy, B * cx + C * cy
        keep[:, q] = live & (ax <= hx) & (ay <= hy) & (cx * t1 + cy * t2 - 3.0 * (np.abs(t1) + np.abs(t2)) <= tau)
    return keep


def pixel_alpha(ids, tx0, ty0):
    X, Y = (tx0 + PX).reshape(-1), (ty0 + PY).reshape(-1)
    dx, dy = uv[ids, 0:1] - X[None, :], uv[ids, 1:2] - Y[None, :]
    power = -0.5 * (conic[ids, 0:1] * dx * dx + conic[ids, 2:3] * dy * dy) - conic[ids, 1:2] * dx * dy
    a = np.minimum(0.99, op[ids, None] * np.exp(power))
    return np.where((power <= 0.0) & (a >= 1.0 / 255.0), a, 0.0)


# ---- 1. quarters per pair
rng = np.random.default_rng(0)
tot = dict(pairs=0, rule=0, pixel=0)
for i in rng.choice(N, NG, replace=False):
    r = radius[i]
    if r <= 0:
        continue
    x0 = min(gx, max(0, int((uv[i, 0] - r) / 16))); x1 = min(gx, max(0, int((uv[i, 0] + r + 15) / 16)))
    y0 = min(gy, max(0, int((uv[i, 1] - r) / 16))); y1 = min(gy, max(0, int((uv[i, 1] + r + 15) / 16)))
    for ty in range(y0, y1):
        for tx in range(x0, x1):
            ids = np.array([i])
            tot["pairs"] += 1
            tot["rule"] += int(rule_quarters(ids, 16.0 * tx, 16.0 * ty).sum())
            tot["pixel"] += int(((pixel_alpha(ids, 16.0 * tx, 16.0 * ty) > 0) @ ONEHOT > 0).sum())
print("1. quarters per reference pair:", {k: round(v / tot["pairs"], 3) for k, v in tot.items() if k != "pairs"},
      "pixel-exact / rule = %.4f" % (tot["pixel"] / tot["rule"]))

# ---- 2. steps of the backward on sampled tiles
vis = depth.reshape(-1) != 0
idx, tr = oracle.sort_gaussian(uv.astype(np.float32), depth, W, H, radius, tiles)
steps = dict(rule=0, applied=0)
coupled = dict(rule=0, applied=0)
entries = dict(rule=0, applied=0)
lens = []
for t in rng.choice(gx * gy, NT, replace=False):
    b, e = int(tr[t, 0]), int(tr[t, 1])
    L = e - b
    if L == 0:
        continue
    ids = idx[b:e]
    tx0, ty0 = 16.0 * (t % gx), 16.0 * (t // gx)
    alpha = pixel_alpha(ids, tx0, ty0)
    inside = ((tx0 + PX) < W).reshape(-1) & ((ty0 + PY) < H).reshape(-1)
    T, done, stop_at, last = np.ones(256), ~inside, np.where(inside, L, -1), 0
    app = np.zeros((L, 256), bool)
    for i in range(L):
        act = ~done & (alpha[i] > 0)
        test = T * (1.0 - alpha[i])
        stop = act & (test < 1e-4)
        ap = act & ~stop
        T = np.where(ap, test, T)
        stop_at[stop] = i
        done |= stop
        app[i] = ap
        if ap.any():
            last = i + 1
        if done.all():
            break
    qdone = np.array([stop_at[QOF == q].max() for q in range(16)])        # the quarter's last pixel stopped at this entry
    rule = rule_quarters(ids, tx0, ty0)
    base = (np.arange(L) // SB) * SB                                        # the forward drops a quarter at the super-batch after
    rule &= qdone[None, :] >= base[:, None]
    words = dict(rule=rule[:last], applied=(app[:last].astype(np.float64) @ ONEHOT) > 0)
    lens.append(last)
    for k, wd in words.items():
        for top in range(last, 0, -SB):
            cnt = wd[max(top - SB, 0):top].sum(0)
            st = (cnt + 15) // 16
            steps[k] += int(st.sum())
            entries[k] += int(cnt.sum())
            coupled[k] += int(max(st[WAVE_OF_Q == w].sum() for w in range(4)))
print("2. %d tiles, mean walked list length %.0f" % (len(lens), np.mean(lens)))
for k in ("rule", "applied"):
    print("   %-8s steps %d  coupled %d  fill %.3f" % (k, steps[k], coupled[k], entries[k] / (16.0 * steps[k])))
print("   applied / rule: steps %.4f, coupled %.4f" % (steps["applied"] / steps["rule"], coupled["applied"] / coupled["rule"]))
