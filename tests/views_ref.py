"""numpy restatement of the display-ready bytes of splatter_a_video_amd.views (test infrastructure; kernel: csrc/views.hip).

``to_uint8``: the reference's ``(x.clamp(0, 1) * 255).astype(np.uint8)`` (src/trainer_fragGS.py:1151-1152) in float32, a NaN -> 0.
``anaglyph``: both eyes clamped, ``o_c = ((((m0 l_r + m1 l_g) + m2 l_b) + m3 r_r) + m4 r_g) + m5 r_b`` with every product and sum
rounded to float32 once (numpy rounds every float32 operation; nothing is contracted), byte = trunc(min(max(o_c * 255, 0), 255)).
``anaglyph_f64``: the reference's own formula (:1250-1253): float32 clamped images, the einsum and the * 255 in float64."""
import numpy as np


def clamp01(x):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(x > 0, x, np.float32(0))           # (a NaN compares false: 0)
        return np.where(v < 1, v, np.float32(1)).astype(np.float32)


def to_uint8(images):
    """[T,3,H,W] float32 -> [T,H,W,3] uint8"""
    v = clamp01(images) * np.float32(255.0)
    assert v.dtype == np.float32
    return np.ascontiguousarray(v.astype(np.uint8).transpose(0, 2, 3, 1))


def anaglyph(left, right, m):
    """[T,3,H,W] x 2, m [3,6] -> [T,H,W,3] uint8, float32 throughout"""
    m = np.asarray(m, np.float32).reshape(3, 6)
    l, r = clamp01(left), clamp01(right)
    ch = [l[:, 0], l[:, 1], l[:, 2], r[:, 0], r[:, 1], r[:, 2]]
    out = []
    for c in range(3):
        o = m[c, 0] * ch[0]
        for k in range(1, 6):
            o = o + m[c, k] * ch[k]
        assert o.dtype == np.float32
        s = o * np.float32(255.0)
        s = np.minimum(np.maximum(s, np.float32(0)), np.float32(255))
        out.append(s.astype(np.uint8))
    return np.ascontiguousarray(np.stack(out, axis=-1))


def anaglyph_f64(left, right, m):
    """the reference: img_cat [H,W,6] float32 (clamped), m float64 [3,6], einsum and * 255 in float64, astype(uint8)"""
    m = np.asarray(m, np.float64).reshape(3, 6)
    cat = np.concatenate([clamp01(left), clamp01(right)], axis=1).transpose(0, 2, 3, 1)     # [T,H,W,6]
    img = np.einsum("tijk,lk->tijl", cat, m)
    return (np.clip(img, 0.0, 1.0) * 255).astype(np.uint8)
