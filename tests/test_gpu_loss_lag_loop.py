"""The epoch loop of models.py lets its losses lag one launch (Engine.set_loss_lag) so that its steps may defer their dense update.
The lag must end with the loop, however the loop ends: afterwards a step asked for its loss (train_step, Engine.step) returns ITS
OWN loss at once, nothing is left pending, and no pending record points into the loop's loss buffer.

Shape: VBPR, U = 300, I = 400, D = 256, d = 12, k = 16, bf16, sgd, batch 512 (2B >= I: segment-mode steps, which defer).
The check of "its own loss": the same step from the same restored state on the same engine, asked for its loss in the plain way
(never lagging), gives the same value up to the summation order of the sparse kernels (1e-5 relative: fp32 sums of 512 terms),
while the loss of the previous step -- what a lagging read would return -- is taken on another batch and differs by far more."""
from argparse import Namespace

import numpy as np
import pytest

from fashionvisualexpl_recommend_amd import configs, synth

pytestmark = pytest.mark.gpu

U, I, D, B = 300, 400, 256, 512


def _model(tmp_path):
    from fashionvisualexpl_recommend_amd.dataset import DataLoader
    from fashionvisualexpl_recommend_amd.models import VBPR
    tr, va, te = synth.make_interactions_clustered(U, I, per_user=14, clusters=10, p_in=0.9, seed=11)
    rs = np.random.RandomState(3)
    feats = (np.abs(rs.standard_normal((I, D))) * (rs.rand(I, D) < 0.5) * 3.7).astype(np.float64)
    synth.write_dataset(str(tmp_path), "lag", tr, va, te, I, features=feats)
    configs.set_roots(str(tmp_path), str(tmp_path / "results"))
    params = Namespace(dataset="lag", validation=True, batch_size=B, epochs=2, batch_eval=128, embed_k=16, embed_d=12, lr=0.05,
                       reg=1e-3, top_k=10, verbose=-1, restore_epochs=1, rec="vbpr", best_metric="ndcg", optimizer="sgd",
                       init_seed=0, dtype="bf16", cnn_model="vgg19", output_layer="fc2")
    return VBPR(DataLoader(params), params)


def _batch(seed):
    rs = np.random.RandomState(seed)
    return rs.randint(U, size=B).astype(np.int32), rs.randint(I, size=B).astype(np.int32), rs.randint(I, size=B).astype(np.int32)


def _own_loss_after(model):
    e = model.engine
    assert not e.dense_pending()
    model.train_step(_batch(1))                             # the step before: a lagging read would return ITS loss
    assert not e.dense_pending()                            # asked for its loss: today's sequence, nothing deferred
    state = model.state_dict()
    got = model.train_step(_batch(2))
    other = model.train_step(_batch(3))
    model.load_state_dict(state)
    want = model.train_step(_batch(2))
    assert np.isfinite(got) and got > 0.0
    assert got == pytest.approx(want, rel=1e-5), (got, want)
    assert abs(other - want) > 1e-3 * want                  # (the check can tell two steps apart)


def test_train_step_after_a_lagged_loop_returns_its_own_loss(tmp_path, monkeypatch):
    monkeypatch.setenv("BPRX_DENSE_DEFER", "1")
    model = _model(tmp_path)
    e = model.engine
    seen = []
    real = e.step

    def spy(*a, **kw):
        r = real(*a, **kw)
        seen.append(e.dense_pending())
        return r
    monkeypatch.setattr(e, "step", spy)
    results = model.train()
    monkeypatch.setattr(e, "step", real)
    # the loop's full batches did defer (an epoch's short last batch is a list-mode step, which never does)
    assert sorted(results) == [1, 2] and sum(seen) >= len(seen) // 2 > 0, seen
    _own_loss_after(model)
    e.close()


def test_a_loop_that_raises_leaves_nothing_pending(tmp_path, monkeypatch):
    monkeypatch.setenv("BPRX_DENSE_DEFER", "1")
    model = _model(tmp_path)

    def boom(*a, **kw):
        raise RuntimeError("evaluator failed")
    monkeypatch.setattr(model.evaluator, "eval", boom)
    with pytest.raises(RuntimeError, match="evaluator failed"):
        model.train()
    _own_loss_after(model)
    model.engine.close()
