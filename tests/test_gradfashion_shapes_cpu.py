"""The inputs of tests/test_gpu_gradfashion_shapes.py on the float64 restatement, without a GPU: no score difference near the
clip, no table with a zero gradient, float32 rounding far inside the bounds the GPU is held to -- and the control that shows
those bounds would catch a step computed from stale [E|Bp]^T images."""
import numpy as np
import pytest
import torch

import gradfashion_shapes as S
from gradfashion_ref import PARAMS, GradFashionRef

CASES = [(n, dt) for n in S.SHAPES for dt in ("fp32", "bf16")]


def test_additive_dtype_argument():
    t, _, _ = S.case("tiny", "fp32")
    assert GradFashionRef(t, reg=0.1).p["Ec"].dtype == torch.float64
    r = GradFashionRef(t, reg=0.1, dtype=torch.float32)
    assert all(v.dtype == torch.float32 for v in r.p.values()) and r.Fc.dtype == torch.float32 and r.m["E"].dtype == torch.float32
    np.testing.assert_array_equal(r.p["Ec"].numpy(), t["Ec"])


@pytest.mark.parametrize("name,dtype", CASES)
def test_scores_stay_clear_of_the_clip(name, dtype):
    """Every score difference of every batch lies in (-40, 40): the clip at -80 and its gradient mask are never near."""
    t, F, batches = S.case(name, dtype)
    Dc, De = S.shape_of(name)[:2]
    assert F.shape == (S.I, S.pad(Dc, De, dtype)) and not F[:, Dc + De:].any()
    ref = GradFashionRef(t, reg=S.REG)
    for u, i, j in batches:
        diff = ref.call(u, i)[0] - ref.call(u, j)[0]
        assert float(diff.abs().max()) < 40.0, float(diff.abs().max())
    _, _, after = S.run_sgd(t, batches)                                 # ... and after the steps the GPU tests take
    u, i, j = batches[-1]
    assert float((after.call(u, i)[0] - after.call(u, j)[0]).abs().max()) < 40.0


@pytest.mark.parametrize("name,dtype", CASES)
def test_every_table_moves_and_float32_is_far_inside_the_bounds(name, dtype):
    t, _, batches = S.case(name, dtype)
    l64, g, r64 = S.run_sgd(t, batches[:1])
    l32, _, r32 = S.run_sgd(t, batches[:1], dtype=torch.float32)
    t64, t32 = S.tables_of(r64), S.tables_of(r32)
    for n in PARAMS:
        assert g[0][n] > 0, n
        dev, bound = float(np.abs(t32[n] - t64[n]).max()), S.table_bound("fp32", S.LR, g[0][n])
        assert dev <= bound / 10, (n, dev, bound)
    assert abs(l32[0] - l64[0]) <= S.LOSS_REL["fp32"] * abs(l64[0]) / 10, (l32[0], l64[0])


@pytest.mark.parametrize("name", S.STALE_SHAPES)
def test_stale_images_would_break_the_bf16_bounds(name):
    """A second step computed from the images built before the first one moves Tu's gradient by more than 10x what the bf16 table
    bound (2e-2 of max|g|) allows, and, on the base and bench shapes, the loss by more than 10x its bound of 1e-3."""
    t, _, batches = S.case(name, "bf16")
    dg, dl = S.stale_control(t, batches)
    print("%s: stale images move g_Tu by %.3g of max|g_Tu|, the loss by %.3g" % (name, dg, dl))
    assert dg >= 10 * 2e-2, dg
    if name != "exact":
        assert dl >= 10 * S.LOSS_REL["bf16"], dl
