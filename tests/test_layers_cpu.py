"""Layer editing without a GPU: splat_frame_preprocess_layer_batch and splat_layer_centroids (csrc/preprocess.hip) exported,
declared, listed and refusing bad arguments with SPLAT_E_ARG before any HIP call (additions only: the ABI version stays 22);
the argument validation of Layer / LayeredClip / render_part / add_foreground on CPU tensors; foreground_mask against the
reference's two expressions; tests/layers_ref.py against a direct torch transcription of add_fg's cat / mean / scale lines
(reference src/trainer_fragGS.py:1344-1387); and the quaternion round trip of :1365-1371, which returns +-q."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import layers_ref as LR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PRE = "splat_frame_preprocess_layer_batch"
CEN = "splat_layer_centroids"
ONE = ctypes.c_void_p(16)          # never dereferenced: every call of these tests is refused on the host or launches nothing
F32 = ctypes.c_float


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L


def test_symbols_are_exported_declared_listed_and_the_abi_version_stays(L):
    so = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    declared = set(re.findall(r"\b(splat_[a-z0-9_]+)\s*\(", header))
    for name in (PRE, CEN, CEN + "_scratch_bytes"):
        assert name in L.SYMBOLS and hasattr(so, name) and name in declared, name
    lib = L.lib()
    assert len(lib.splat_frame_preprocess_layer_batch.argtypes) == 31
    assert len(lib.splat_layer_centroids.argtypes) == 13
    assert lib.splat_abi_version() == 22 and L.ABI_VERSION == 22
    assert re.search(r"#define SPLAT_ABI_VERSION 22\b", header)
    doc = header[header.index("---- layer editing"):][:3500]
    assert "No float atomics" in doc and "bit for bit" in doc and "trainer_fragGS.py:1310-1405" in doc
    import splatter_a_video_amd as pkg
    for name in ("Layer", "LayeredClip", "render_part", "add_foreground", "foreground_mask"):
        assert hasattr(pkg, name), name
    # 64 lanes x 16 elements per block, three float64 sums per block and frame
    assert lib.splat_layer_centroids_scratch_bytes(6, 345) == 6 * 1 * 24
    assert lib.splat_layer_centroids_scratch_bytes(2, 1025) == 2 * 2 * 24
    assert lib.splat_layer_centroids_scratch_bytes(0, 5) == 0 and lib.splat_layer_centroids_scratch_bytes(5, 0) == 0


def _pre(lib, **k):
    a = dict(F=6, P=100, S=40, Q=140, q0=100, I=4, tab=ONE, src=ONE, position=ONE, cubic=ONE, layout=1, rotation=ONE, rot_poly=ONE,
             rot_fourier=ONE, opacity=ONE, scaling=ONE, extr=ONE, W=96, H=64, centroid=None, delta=None, scale=1.0, splats=0, uv=ONE,
             depth=ONE, conic=ONE, radius=ONE, opa_t=ONE)
    a.update(k)
    return lib.splat_frame_preprocess_layer_batch(
        a["F"], a["P"], a["S"], a["Q"], a["q0"], a["I"], a["tab"], a["src"], a["position"], a["cubic"], a["layout"], a["rotation"],
        a["rot_poly"], a["rot_fourier"], a["opacity"], a["scaling"], a["extr"], a["W"], a["H"], F32(0.01), F32(1.3), a["centroid"],
        a["delta"], F32(a["scale"]), a["splats"], a["uv"], a["depth"], a["conic"], a["radius"], a["opa_t"], None)


def test_layer_preprocess_validates_before_hip(L):
    lib = L.lib()
    err = lib.splat_last_error
    assert _pre(lib, P=0) == -1 and b"sizes" in err() and PRE.encode() in err()
    for bad in (dict(F=-1), dict(F=65536), dict(S=-2), dict(Q=0), dict(q0=-1), dict(I=0), dict(W=0), dict(H=-3)):
        assert _pre(lib, **bad) == -1 and b"sizes" in err(), bad
    assert _pre(lib, S=101, Q=300) == -1 and b"at most P" in err()
    assert _pre(lib, q0=101) == -1 and b"q0 + S" in err()                 # 101 + 40 > 140
    assert _pre(lib, q0=0x7fffffff, Q=0x7fffffff) == -1 and b"q0 + S" in err()   # no int overflow in the sum
    assert _pre(lib, layout=7) == -1 and b"cubic_layout" in err()
    for s in (float("nan"), float("inf"), float("-inf")):
        assert _pre(lib, scale=s, centroid=ONE) == -1 and b"finite" in err(), s
    assert _pre(lib, scale=0.6) == -1 and b"centroid" in err()            # scale != 1 needs the centroid
    assert _pre(lib, scale=0.6, delta=ONE) == -1 and b"centroid" in err()
    assert _pre(lib, src=None) == -1 and b"S must be P" in err()          # src == NULL only with S == P
    for k in ("tab", "position", "cubic", "rotation", "rot_poly", "rot_fourier", "opacity", "scaling", "extr"):
        assert _pre(lib, **{k: None}) == -1 and b"null input" in err(), k
    for k in ("uv", "depth", "conic", "radius", "opa_t"):
        assert _pre(lib, **{k: None}) == -1 and b"null output" in err(), k
    # S == 0 or F == 0 is valid and launches nothing (no HIP call: this machine has no GPU)
    assert _pre(lib, S=0) == 0 and _pre(lib, F=0) == 0
    assert _pre(lib, S=0, scale=0.5, centroid=ONE, delta=ONE, splats=1) == 0


def _cen(lib, **k):
    a = dict(F=6, P=100, S=40, I=4, tab=ONE, src=ONE, position=ONE, cubic=ONE, layout=0, centroid=ONE, scratch=ONE, nbytes=1 << 20)
    a.update(k)
    return lib.splat_layer_centroids(a["F"], a["P"], a["S"], a["I"], a["tab"], a["src"], a["position"], a["cubic"], a["layout"],
                                     a["centroid"], a["scratch"], a["nbytes"], None)


def test_layer_centroids_validates_before_hip(L):
    lib = L.lib()
    err = lib.splat_last_error
    assert _cen(lib, P=0) == -1 and b"sizes" in err() and CEN.encode() in err()
    for bad in (dict(F=-1), dict(F=65536), dict(S=-1), dict(I=0)):
        assert _cen(lib, **bad) == -1 and b"sizes" in err(), bad
    assert _cen(lib, S=101) == -1 and b"at most P" in err()
    assert _cen(lib, layout=2) == -1 and b"cubic_layout" in err()
    assert _cen(lib, src=None) == -1 and b"S must be P" in err()
    for k in ("tab", "position", "cubic"):
        assert _cen(lib, **{k: None}) == -1 and b"null input" in err(), k
    assert _cen(lib, centroid=None) == -1 and b"null output" in err()
    assert _cen(lib, scratch=None) == -1 and b"scratch" in err()
    assert _cen(lib, scratch=ctypes.c_void_p(20)) == -1 and b"aligned" in err()
    assert _cen(lib, nbytes=6 * 24 - 1) == -1 and b"too small" in err()
    assert _cen(lib, S=0) == 0 and _cen(lib, F=0) == 0 and _cen(lib, S=0, scratch=None, nbytes=0) == 0


# ------------------------------------------------------------------ python validation on CPU tensors
def _model(N=5, T=8):
    from splatter_a_video_amd.dynamics import FrameClock
    clock = FrameClock(T)
    I = clock.interval_num
    model = {"position": torch.zeros(N, 3), "pos_cubic_node": torch.zeros(N, 4 * I * 3), "rotation": torch.ones(N, 4),
             "rot_poly_feat": torch.zeros(N, 4, 4), "rot_fourier_feat": torch.zeros(N, 8, 4), "opacity": torch.zeros(N, 1),
             "scaling": torch.zeros(N, 3), "shs": torch.zeros(N, 16, 3),
             "mask_attribute": torch.tensor([[0.9], [0.1], [0.7], [0.5], [float("nan")]])[:N]}
    return clock, model


def test_layer_validation():
    from splatter_a_video_amd.layers import Layer
    l_ = Layer()
    assert l_.select is None and l_.times is None and l_.scale == 1.0 and l_.delta is None and not l_.scale_splats and not l_.transformed
    assert Layer(scale=0.5).transformed and Layer(delta=[0.0, 0.0, 0.0]).transformed and not Layer(scale_splats=True).transformed
    assert Layer(delta=torch.zeros(4, 3)).delta.shape == (4, 3) and Layer(times=[3, 1, 1, 0]).times == [3.0, 1.0, 1.0, 0.0]
    with pytest.raises(TypeError, match="select"):
        Layer(select=[True, False])
    for bad in (torch.ones(4), torch.ones(2, 2, dtype=torch.bool)):
        with pytest.raises(ValueError, match="select"):
            Layer(select=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            Layer(scale=bad)
    with pytest.raises(TypeError, match="scale"):
        Layer(scale="2")
    for bad in ([1.0, 2.0], torch.zeros(3, 2), torch.zeros(2, 3, 1), torch.zeros(0, 3)):
        with pytest.raises(ValueError, match="delta"):
            Layer(delta=bad)
    with pytest.raises(ValueError, match="finite"):
        Layer(delta=[0.0, float("nan"), 0.0])
    with pytest.raises(ValueError, match="finite"):
        Layer(times=[0.0, float("inf")])


def test_layered_clip_validation():
    from splatter_a_video_amd.layers import Layer, LayeredClip
    N, W, H = 5, 32, 16
    clock, model = _model(N)
    extr = torch.eye(4)
    sel = torch.tensor([True, False, True, False, False])
    sets = [dict(feature=torch.zeros(N, 3), bg=1.0), dict(feature="depth", bg=1.0)]
    call = lambda m=model, layers=None, e=extr, s=sets, **k: LayeredClip(m, clock, [Layer(select=sel)] if layers is None else layers,
                                                                          e, k.pop("W", W), k.pop("H", H), s, **k)
    for bad, match in ((dict(layers=[]), "non-empty list"), (dict(layers=[Layer()] * 17), "at most 16 layers"),
                       (dict(layers=[Layer(select=torch.zeros(N, dtype=torch.bool))]), "selection is empty"),
                       (dict(layers=[Layer(), Layer(select=torch.ones(N + 1, dtype=torch.bool))]), r"layer 1: select must be \[N = 5\]"),
                       (dict(W=0), "W and H"), (dict(H=-1), "W and H"), (dict(frames_per_batch=0), "frames_per_batch"),
                       (dict(frames_per_batch=2.5), "frames_per_batch"), (dict(capacity=0), "capacity"), (dict(K=4), "K > 0"),
                       (dict(e=torch.eye(3)), "extr"), (dict(e=torch.zeros(2, 4, 4)), "extr"), (dict(s=[]), "sets"),
                       (dict(s=[dict(feature=torch.zeros(N + 1, 3))]), r"\[N = 5, c\]"), (dict(s=[dict(feature=torch.zeros(N))]), r"\[N = 5, c\]"),
                       (dict(s=[dict(feature="normal")]), '"depth"'), (dict(s=[dict(feature=torch.zeros(N, 3, dtype=torch.float64))]), "float32"),
                       (dict(s=[dict(feature=torch.zeros(N, 30)), dict(feature=torch.zeros(N, 3))]), "33 channels"),
                       (dict(cubic_layout=5), "cubic_layout")):
        with pytest.raises(ValueError, match=match):
            call(**bad)
    with pytest.raises(TypeError, match="list of Layer"):
        call(layers=[dict(select=sel)])
    with pytest.raises(TypeError, match="dict with a 'feature'"):
        call(s=[torch.zeros(N, 3)])
    with pytest.raises(TypeError, match="parameter dict or DynamicGaussians"):
        call(m=[1, 2])
    with pytest.raises(ValueError, match="lacks"):
        call(m={k: v for k, v in model.items() if k != "scaling"})
    with pytest.raises(ValueError, match="model rotation does not hold"):
        call(m={**model, "rotation": torch.ones(N + 1, 4)})
    noshs = {k: v for k, v in model.items() if k != "shs"}          # explicit feature sets need no SH coefficients
    for m in (model, noshs):
        with pytest.raises(ValueError, match="CUDA"):               # well-formed arguments still need the GPU: no CPU path
            call(m=m)
    with pytest.raises(ValueError, match="CUDA"):                   # 32 channels are the limit, not an error
        call(s=[dict(feature=torch.zeros(N, 31)), dict(feature="depth")])


def test_clip_length_checks():
    from splatter_a_video_amd.layers import Layer, clip_layer_inputs
    layers = [Layer(), Layer(times=[2, 0, 0], scale=0.5, delta=[1.0, 2.0, 3.0]), Layer(delta=torch.ones(3, 3))]
    times, lt, ld = clip_layer_inputs(layers, [4, 5, 6])
    assert times == [4.0, 5.0, 6.0] and lt == [[4.0, 5.0, 6.0], [2.0, 0.0, 0.0], [4.0, 5.0, 6.0]]
    assert ld[0] is None and ld[1].shape == (3, 3) and torch.equal(ld[1][2], torch.tensor([1.0, 2.0, 3.0])) and ld[2].shape == (3, 3)
    with pytest.raises(ValueError, match="layer 1: 3 times for a clip of 4 frames"):
        clip_layer_inputs(layers, [0, 1, 2, 3])
    with pytest.raises(ValueError, match=r"layer 1: delta must be \[3\] or \[T_clip = 2, 3\]"):
        clip_layer_inputs([Layer(), Layer(delta=torch.ones(3, 3))], [0, 1])
    with pytest.raises(ValueError, match="at least one frame time"):
        clip_layer_inputs(layers, [])


def test_wrappers_validate_before_gpu_work():
    from splatter_a_video_amd.layers import add_foreground, render_part
    N, W, H = 5, 32, 16
    clock, model = _model(N)
    extr, times = torch.eye(4), [0, 1, 2]
    part = lambda m=model, **k: render_part(m, clock, times, extr, W, H, **k)
    add = lambda m=model, delta=(0.1, 0.0, 0.0), scale=0.5, **k: add_foreground(m, clock, times, extr, W, H, delta, scale, **k)
    for call in (part, add):
        with pytest.raises(ValueError, match="pass shs="):
            call(m={k: v for k, v in model.items() if k != "shs"})
        with pytest.raises(ValueError, match=r"shs must be \[N = 5, 16, 3\]"):
            call(shs=torch.zeros(N, 4, 3))
        with pytest.raises(ValueError, match="pass mask_attribute="):
            call(m={k: v for k, v in model.items() if k != "mask_attribute"})
        with pytest.raises(ValueError, match=r"mask_attribute must be \[N = 5\]"):
            call(mask_attribute=torch.zeros(N + 2))
        with pytest.raises(ValueError, match="frames_per_batch"):
            call(frames_per_batch=0)
        with pytest.raises(ValueError, match="CUDA"):
            call()
        with pytest.raises(ValueError, match="CUDA"):               # the mask as an argument, [N]
            call(m={k: v for k, v in model.items() if k != "mask_attribute"}, mask_attribute=model["mask_attribute"][:, 0])
    with pytest.raises(ValueError, match="selection is empty"):
        part(threshold=2.0)
    with pytest.raises(ValueError, match="selection is empty"):
        part(fg=False, threshold=-1.0)
    with pytest.raises(ValueError, match="selection is empty"):
        add(fg_threshold=2.0)
    for bad, match in ((dict(delta=(0.1, 0.2)), "delta must be"), (dict(scale=float("nan")), "finite"), (dict(delay=-1), "delay"),
                       (dict(drift=(1.0,)), "drift must be")):
        with pytest.raises(ValueError, match=match):
            add(**bad)


def test_foreground_mask_is_the_references_two_expressions():
    from splatter_a_video_amd.layers import foreground_mask
    gen = torch.Generator().manual_seed(3)
    m = torch.rand(200, 1, generator=gen)
    m[7], m[8], m[9] = 0.5, float("nan"), 0.25
    for thr in (0.5, 0.25, 0.9):
        fg, bgm = foreground_mask(m, thr, True), foreground_mask(m, thr, False)
        assert torch.equal(fg, m.squeeze() > thr) and torch.equal(bgm, m.squeeze() <= thr)       # (:1320, :1322)
        assert fg.dtype == torch.bool and fg.shape == (200,)
        assert not fg[8] and not bgm[8]                                 # a NaN falls in neither
        assert int(fg.sum()) + int(bgm.sum()) == 199
    assert not foreground_mask(m, 0.5)[7] and foreground_mask(m, 0.5, fg=False)[7]              # the threshold itself: background
    assert torch.equal(foreground_mask(m[:, 0]), foreground_mask(m))
    with pytest.raises(ValueError, match=r"\[N\] or \[N, 1\]"):
        foreground_mask(torch.zeros(4, 2))


# ------------------------------------------------------------------ the numpy restatement against a torch transcription
def _host(N, T, seed):
    from splatter_a_video_amd.dynamics import FrameClock
    clock = FrameClock(T)
    I = clock.interval_num
    rng = np.random.default_rng(seed)
    f = lambda *s, scale=1.0: rng.normal(0, scale, size=s).astype(np.float32)
    host = dict(position=np.concatenate([rng.uniform(-1.1, 1.1, size=(N, 2)), rng.uniform(2.0, 4.0, size=(N, 1))], 1).astype(np.float32),
                pos_cubic_node=f(N, 4 * I * 3, scale=0.02), rotation=f(N, 4), rot_poly_feat=f(N, 4, 4, scale=0.05),
                rot_fourier_feat=f(N, 8, 4, scale=0.05), opacity=f(N, 1, scale=1.5),
                scaling=np.log(rng.uniform(0.006, 0.03, size=(N, 3))).astype(np.float32))
    return clock, host, rng


def test_layers_ref_against_a_torch_transcription_of_add_fg(oracle_mod):
    N, T = 50, 12
    clock, host, rng = _host(N, T, 2)
    mask_attr = rng.uniform(size=(N, 1)).astype(np.float32)
    rgb = rng.uniform(size=(N, 3)).astype(np.float32)
    fg = mask_attr[:, 0] > 0.5
    assert 10 < fg.sum() < 40
    times = [0, 3, 7, 11]
    delta0, drift, scale = np.array([[0.45, -0.3, -0.5]], np.float32), np.array([[-0.01, 0.0, 0.02]], np.float32), 0.6
    ltimes = [max(0, t - 2) for t in times]
    deltas = np.stack([(torch.tensor(delta0).clone() + torch.tensor(drift) * lt).numpy()[0] for lt in ltimes])     # (:1354-1355)
    layers = [dict(select=None), dict(select=fg, times=ltimes, scale=scale, delta=deltas)]
    fg_mask = torch.tensor(fg)
    for f, (t, lt) in enumerate(zip(times, ltimes)):
        got = LR.frame_arrays(oracle_mod, clock, host, layers, times, f, features=[rgb, mask_attr])
        ev = lambda tt: dict(zip(("position", "rotation", "opacity", "scaling"),
                                 (torch.tensor(a) for a in LR.evaluate(oracle_mod, clock, host, tt))))
        render_dict, render_dict_tmp = ev(t), ev(lt)
        for d_ in (render_dict, render_dict_tmp):
            d_["rgb"], d_["mask_attribute"] = torch.tensor(rgb), torch.tensor(mask_attr)
        # (:1357-1387) in torch on the CPU
        fg_pos = render_dict_tmp["position"][fg_mask]
        fg_pos_mean = fg_pos.mean(dim=0, keepdim=True)
        fg_pos = (fg_pos - fg_pos_mean) * scale + fg_pos_mean
        fg_pos = fg_pos + torch.tensor(deltas[f:f + 1])
        want = {k: torch.cat([v, render_dict_tmp[k][fg_mask]], dim=0) for k, v in render_dict.items() if k != "position"}
        want["position"] = torch.cat([render_dict["position"], fg_pos], dim=0)
        Q = N + int(fg.sum())
        assert got["position"].shape == (Q, 3) and got["position"].dtype == np.float32
        for k, g in (("rotation", got["rotation"]), ("opacity", got["opacity"]), ("scaling", got["scale"]), ("rgb", got["features"][0]),
                     ("mask_attribute", got["features"][1])):
            assert np.array_equal(g, want[k].numpy()), k
        assert np.array_equal(got["position"][:N], want["position"][:N].numpy())        # the base layer: untouched bits
        # the copy: torch's float32 mean against float32(mean in float64) -- a few roundings of a sum of 20-odd terms of size <= 4
        c32, c64 = fg_pos_mean.numpy(), got["centroids"][1]
        assert got["centroids"][0] is None and np.abs(c32 - c64).max() <= 4 * 2.0 ** -23 * 4.0
        err = np.abs(got["position"][N:] - want["position"][N:].numpy()).max()
        assert err <= 2 * np.abs(c32 - c64).max() + 2.0 ** -23 * 4.0, err
    # scale_splats multiplies the activated scale; a [3] delta is every frame's
    l2 = [dict(select=fg, scale=1.4, delta=delta0[0], scale_splats=True)]
    a = LR.frame_arrays(oracle_mod, clock, host, l2, times, 1)
    _, _, _, scl = LR.evaluate(oracle_mod, clock, host, times[1])
    assert np.array_equal(a["scale"], (scl[fg] * np.float32(1.4)).astype(np.float32))
    # an untransformed selection is the masked rows (render_part, :1323)
    b = LR.frame_arrays(oracle_mod, clock, host, [dict(select=~fg)], times, 2)
    pos, rot, opa, scl = LR.evaluate(oracle_mod, clock, host, times[2])
    assert np.array_equal(b["position"], pos[~fg]) and np.array_equal(b["rotation"], rot[~fg]) and b["centroids"] == [None]


def test_quaternion_round_trip_returns_plus_or_minus_q():
    """(:1365-1371) quaternion_to_matrix -> matrix_to_quaternion -> normalise gives +-q: |q - sign q'| <= 1e-6, a few float32
    roundings of a unit quaternion"""
    sys.path.insert(1, os.path.join(ROOT, "shims"))
    try:
        from pytorch3d import transforms
        gen = torch.Generator().manual_seed(5)
        q = torch.randn(2001, 4, generator=gen)
        q = q / q.norm(dim=-1, keepdim=True)
        q2 = transforms.matrix_to_quaternion(transforms.quaternion_to_matrix(q))
        q2 = q2 / q2.norm(dim=-1, keepdim=True)
    finally:
        sys.path.remove(os.path.join(ROOT, "shims"))
        for m in [m for m in sys.modules if m == "pytorch3d" or m.startswith("pytorch3d.")]:
            del sys.modules[m]
    sign = torch.sign((q * q2).sum(-1, keepdim=True))
    err = float((q - sign * q2).abs().max())
    print(f"quaternion round trip: max |q - sign q'| = {err:.3e}, negated {float((sign < 0).float().mean()):.1%}")
    assert err <= 1e-6
