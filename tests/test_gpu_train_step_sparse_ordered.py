"""TrainingStep(sparse_track=True, ordered_track=True): the sparse track term with the ordered backward
(splat_alpha_blending_points_backward_batch_ordered) -- the step runs under the deterministic flag and is bit-reproducible.

Bits: two fresh steps from the same start, seeds and pairs, three steps each under L.set_deterministic(True): every bucket gradient
after the first step and flat_param after the third are torch.equal.  Values: one ordered step against one unordered sparse step
(flag off) under the bound of tests/test_gpu_train_step_sparse_track.py (`_assert_doubled`: both are float32 sums of the same
addends in another order), losses to rtol 1e-5.  Sizes: those of test_one_sparse_step_is_the_dense_step."""
import numpy as np
import pytest
import torch

from splatter_a_video_amd import _lib as L
from splatter_a_video_amd import train_step as TS
from test_gpu_track_loss import _step_tracks
from test_gpu_train_step import _clip, _perturbed, _t
from test_gpu_train_step_sparse_track import REFERENCE, H, T, W, _assert_doubled

pytestmark = pytest.mark.gpu

N, F = 3000, 4
T1, T2 = [0, 3, 7, 12], [5, 1, 19, 2]
GRADS = ("pos_cubic_node", "rotation", "opacity", "scaling", "shs")


def _setup():
    sc, clock, truth = _clip(N, W, H, T, seed=11)
    extr = _t(sc.extr)
    start = _perturbed(truth, 3)
    gt = TS.render_ground_truth(truth, clock, W, H, extr, T1, T2)
    gt["tracks"] = _step_tracks(gt, 4, seed=2, noise=0.5)
    del gt["attr"]                                           # not read by the sparse step
    return clock, extr, start, gt


def _make(clock, extr, start, **kw):
    return TS.TrainingStep(start, clock, W, H, F, extr, K=8, arap_samples=128, sample_seed=4, weights=TS.LossWeights(**REFERENCE),
                           sparse_track=True, **kw)


def test_ordered_sparse_step_is_bit_reproducible_under_the_deterministic_flag():
    clock, extr, start, gt = _setup()
    L.set_deterministic(True)
    try:
        res = []
        for _ in range(2):
            st = _make(clock, extr, start, ordered_track=True)
            st.step(T1, T2, gt)
            torch.cuda.synchronize()
            first = {k: st.bucket.grad(k).detach().clone() for k in TS.TRAINABLE}
            st.step(T1, T2, gt)
            st.step(T1, T2, gt)
            torch.cuda.synchronize()
            res.append((first, st.bucket.flat_param.detach().clone(), st))
    finally:
        L.set_deterministic(False)
    (ga, pa, sa), (gb, pb, sb) = res
    assert sa.iteration == 3 and sb.iteration == 3 and sa.fb.C == 4
    for k in TS.TRAINABLE:
        assert torch.equal(ga[k], gb[k]), f"gradient of {k} after the first step differs between two runs"
    assert all(float(ga[k].abs().max()) > 0 for k in GRADS)
    assert torch.equal(pa, pb), "flat_param after the third step differs between two runs"
    assert not torch.equal(pa, _make(clock, extr, start).bucket.flat_param)


def test_one_ordered_step_is_the_unordered_sparse_step():
    clock, extr, start, gt = _setup()
    res = []
    for ordered in (False, True):
        st = _make(clock, extr, start, ordered_track=ordered)
        last = st.step(T1, T2, gt)
        torch.cuda.synchronize()
        res.append((st, last))
    (a, la), (b, lb) = res
    assert b.ordered_track and not a.ordered_track and set(la) == set(lb)
    for name in GRADS:
        _assert_doubled(b.bucket.grad(name), a.bucket.grad(name), name)
    _assert_doubled(b.dstate.pos_gradient_accum, a.dstate.pos_gradient_accum, "pos_gradient_accum")
    assert float(la["track"]) > 0
    for k in la:
        np.testing.assert_allclose(float(lb[k]), float(la[k]), rtol=1e-5, err_msg=k)


def test_ordered_track_refusals_and_rebuild():
    clock, extr, start, gt = _setup()
    with pytest.raises(ValueError, match="sparse_track"):
        TS.TrainingStep(start, clock, W, H, F, extr, K=8, arap_samples=128, sample_seed=4,
                        weights=TS.LossWeights(**REFERENCE), ordered_track=True)
    cfg = TS.DensifyConfig(interval=2, start_iter=1, cameras_extent=60.0, min_opacity=0.05, seed=123)
    st = _make(clock, extr, start, ordered_track=True, densify=cfg)
    L.set_deterministic(True)
    try:
        st.step(T1, T2, gt)
        assert not st.maybe_densify()
        st.step(T1, T2, gt)
        assert st.maybe_densify()                            # the buffers are rebuilt at the new count
        assert st.ordered_track and st.sparse_track and st.fb.C == 4
        last = st.step(T1, T2, gt)                           # still the ordered entry: the flag does not refuse it
        torch.cuda.synchronize()
    finally:
        L.set_deterministic(False)
    assert st.iteration == 3 and np.isfinite(float(last["track"])) and np.isfinite(st.loss())
