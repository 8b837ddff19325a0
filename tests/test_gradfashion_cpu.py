"""GradFashion without a GPU: the closed-form attribution against autograd's gradient x input, the CLI, the model's host side
(features, normalisation, padding, creation order, directory_parameters) on a stub engine, and the explanation TSV."""
from argparse import Namespace

import numpy as np
import pandas as pd
import pytest
import torch

from fashionvisualexpl_recommend_amd import configs, evaluator, models, synth, train_rec
from gradfashion_ref import GradFashionRef


def _tables(rs, U=7, I=11, k=4, d=3, Dc=5, De=6, ec=2, ee=3):
    return dict(Gu=rs.randn(U, k), Gi=rs.randn(I, k), Bi=rs.randn(I), Tu=rs.randn(U, d), Fc=rs.rand(I, Dc), Fe=rs.rand(I, De),
                Ec=rs.randn(Dc, ec), Ee=rs.randn(De, ee), E=rs.randn(ec + ee, d), Bp=rs.randn(ec + ee, 1))


def test_closed_form_attribution_equals_gradient_times_input():
    ref = GradFashionRef(_tables(np.random.RandomState(3)), reg=0.1)
    pairs = [(u, i) for u in range(7) for i in range(11)]
    got = ref.explain_closed_form([p[0] for p in pairs], [p[1] for p in pairs])
    want = np.concatenate([ref.predict_ui_grads(u, i) for u, i in pairs])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    # colour + edges + the parts that do not depend on the features = the score (the attribution is exact for a linear score)
    p = ref.p
    u, i = torch.tensor([p_[0] for p_ in pairs]), torch.tensor([p_[1] for p_ in pairs])
    rest = p["Bi"][i] + (p["Gu"][u] * p["Gi"][i]).sum(1)
    np.testing.assert_allclose(got.sum(1) + rest.numpy(), ref.call(u, i)[0].detach().numpy(), rtol=1e-12, atol=1e-12)


def test_cli_flags_and_defaults():
    a = train_rec.parse_args(["--rec", "grad_fashion"])
    assert (a.rec, a.embed_color, a.embed_edges, a.embed_d) == ("grad_fashion", 20, 20, 20)
    a = train_rec.parse_args(["--rec", "grad_fashion", "--embed_color", "7", "--embed_edges", "9", "--dtype", "bf16",
                              "--optimizer", "sgd", "--sampler", "philox"])
    assert (a.embed_color, a.embed_edges, a.dtype, a.optimizer, a.sampler) == (7, 9, "bf16", "sgd", "philox")


def test_cli_rejects_multi_gpu():
    with pytest.raises(NotImplementedError, match="grad_fashion"):
        train_rec.train(["--rec", "grad_fashion", "--world_size", "2"])


def test_config_paths():
    configs.set_roots("/data_root", "/res_root")
    try:
        assert configs.hist_color_features_path("ds") == "/data_root/ds/original/features/histograms.npy"
        assert configs.edge_features_path("ds", "resnet50", "avg_pool") == "/data_root/ds/original/edge_features_resnet50_avg_pool.npy"
    finally:
        configs.set_roots("../data", "../results")


class _StubEngine:
    """Records what GradFashion binds (no GPU)."""

    def __init__(self, **kw):
        self.kw = kw
        self.device = torch.device("cpu")

    def bind_factored(self, Gu, Gi, Bi, Tu, F, Ec, Ee, E, Bp, feat_dim_a, feat_dim_b, neg_bias_reg=1.0):
        f = lambda x: torch.as_tensor(x)
        self.t = dict(Gu=f(Gu), Gi=f(Gi), Bi=f(Bi), Tu=f(Tu), F=f(F), Ec=f(Ec), Ee=f(Ee), E=f(E), Bp=f(Bp))
        self.dims = (feat_dim_a, feat_dim_b, neg_bias_reg)
        return self


def _data(U, I, params):
    rs = np.random.RandomState(0)
    tr = [sorted(rs.choice(I, 3, replace=False).tolist()) for _ in range(U)]
    return Namespace(num_users=U, num_items=I, training_list=tr, validation_list=[[u % I] for u in range(U)],
                     test_list=[[(u + 1) % I] for u in range(U)], params=params)


def _params(**kw):
    p = dict(dataset="gf", validation=True, batch_size=64, epochs=1, batch_eval=128, embed_k=8, embed_d=6, embed_color=3,
             embed_edges=4, lr=0.01, reg=0.001, top_k=5, verbose=-1, restore_epochs=1, rec="grad_fashion", best_metric="ndcg",
             optimizer="adam_tf23", init_seed=5, dtype="fp32", cnn_model="vgg19", output_layer="fc2")
    p.update(kw)
    return Namespace(**p)


@pytest.mark.parametrize("dtype,D", [("fp32", 400), ("bf16", 512)])
def test_model_features_padding_and_init(tmp_path, monkeypatch, dtype, D):
    monkeypatch.setattr(models, "Engine", _StubEngine)
    U, I, Dc, De = 9, 13, 100, 290
    rs = np.random.RandomState(1)
    color, edges = rs.rand(I, Dc) * 7.0, -rs.rand(I, De) * 3.0
    synth.write_grad_fashion_features(str(tmp_path), "gf", color, edges)
    configs.set_roots(str(tmp_path), str(tmp_path / "results"))
    try:
        p = _params(dtype=dtype)
        m = models.GradFashion(_data(U, I, p), p)
    finally:
        configs.set_roots("../data", "../results")
    assert m.directory_parameters == "batch_64-D_6-K_8-lr_0.01-reg_0.001"           # GradFashion.py:48-52
    assert (m.embed_color, m.embed_edges, m.dim_color_features, m.dim_edge_features) == (3, 4, Dc, De)
    assert m.engine.kw["feat_dim"] == D and m.engine.kw["feat_dtype"] == dtype and m.engine.kw["model"] == "vbpr"
    assert m.engine.dims == (Dc, De, 1.0)
    F = m.engine.t["F"].numpy()
    np.testing.assert_array_equal(F[:, :Dc], (color / np.abs(color).max()).astype(np.float32))    # each table by its own max
    np.testing.assert_array_equal(F[:, Dc:Dc + De], (edges / np.abs(edges).max()).astype(np.float32))
    assert not F[:, Dc + De:].any()
    np.testing.assert_array_equal(m.color_weights["Fc"].numpy(), F[:, :Dc])
    np.testing.assert_array_equal(m.edges_weights["Fe"].numpy(), F[:, Dc:Dc + De])
    assert tuple(m.visual_profile["Bp"].shape) == (7, 1) and tuple(m.visual_profile["E"].shape) == (7, 6)
    # the reference's creation order: Bi, Gu, Gi, then Bp, E, Tu, then Ec, then Ee (one seeded Glorot stream)
    g = np.random.RandomState(5)
    want = {"Gu": synth.glorot_uniform(g, U, 8), "Gi": synth.glorot_uniform(g, I, 8), "Bp": synth.glorot_uniform(g, 7, 1).reshape(-1),
            "E": synth.glorot_uniform(g, 7, 6), "Tu": synth.glorot_uniform(g, U, 6), "Ec": synth.glorot_uniform(g, Dc, 3),
            "Ee": synth.glorot_uniform(g, De, 4)}
    for n, v in want.items():
        np.testing.assert_array_equal(m.engine.t[n].numpy(), v, err_msg=n)
    assert not m.engine.t["Bi"].numpy().any()


class _ExplainStub:
    def __init__(self):
        self.calls = 0

    def explain_pairs(self, user, item):
        self.calls += 1
        u, i = np.asarray(user, np.float64), np.asarray(item, np.float64)
        return torch.as_tensor(np.stack([u / 7.0 + i, -(u + 1.0) / (i + 3.0)], 1).astype(np.float32))


def test_explanation_tsv_rows_and_format(tmp_path):
    U, I = 10, 20
    p = _params()
    data = _data(U, I, p)
    data.test_list = data.test_list[:U - 1]                  # a short list: the user simply has no test row
    stub = _ExplainStub()
    ev = evaluator.Evaluator(Namespace(engine=stub), data, 5, user_block=4)
    path = str(tmp_path / "recs-1-x.tsv")
    ev.store_recommendation_grads(path)
    assert stub.calls == 3                                    # one device call per block of users, not one per pair
    want = []
    for u in range(U):
        items = data.training_list[u] + data.validation_list[u] + (data.test_list[u] if u < U - 1 else [])
        for i in items:
            c, e = np.float32(u / 7.0 + i), np.float32(-(u + 1.0) / (i + 3.0))
            want.append("%s\t%s\t%s\t%s\n" % (str(u), str(i), str(c), str(e)))
    with open(path) as f:
        assert f.readlines() == want
    df = pd.read_csv(path, sep="\t", names=["USER_ID", "ITEM_ID", "COLOR", "EDGES"])     # get_explanations.py:19-21
    assert len(df) == len(want) and df["USER_ID"].dtype.kind == "i" and df["COLOR"].dtype.kind == "f"
