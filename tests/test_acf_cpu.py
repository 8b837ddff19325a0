"""ACF without a GPU: the CLI flags, the split-features path, loading the per-item feature maps, directory_parameters, creation
order and init distributions on a stub engine, the evaluation histories, and the reference's detached gradient (tests/acf_ref.py)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from acf_ref import ACFRef, random_tables
from fashionvisualexpl_recommend_amd import _ffi, configs, models, train_rec


def test_cli_flags_and_defaults():
    a = train_rec.parse_args(["--rec", "acf"])
    assert (a.rec, a.layers_component, a.layers_item, a.dtype, a.sampler) == ("acf", [64, 1], [64, 1], "fp32", "ref_stream")
    a = train_rec.parse_args(["--rec", "acf", "--layers_component", "32", "1", "--layers_item", "16", "1", "--dtype", "bf16",
                              "--sampler", "philox", "--optimizer", "sgd"])
    assert (a.layers_component, a.layers_item, a.dtype, a.sampler, a.optimizer) == ([32, 1], [16, 1], "bf16", "philox", "sgd")


@pytest.mark.parametrize("bad", [["64"], ["64", "2"], ["64", "1", "1"], ["0", "1"]])
def test_cli_rejects_other_layer_forms(bad):
    with pytest.raises(SystemExit):
        train_rec.parse_args(["--rec", "acf", "--layers_component"] + bad)
    with pytest.raises(SystemExit):
        train_rec.parse_args(["--rec", "acf", "--layers_item"] + bad)


def test_cli_rejects_fp8_and_multi_gpu():
    with pytest.raises(ValueError, match="fp32 or bf16"):
        train_rec.train(["--rec", "acf", "--dtype", "fp8"])
    with pytest.raises(NotImplementedError, match="acf"):
        train_rec.train(["--rec", "acf", "--world_size", "2"])


def test_split_features_path():
    configs.set_roots("/data_root", "/res_root")
    try:
        assert configs.cnn_features_path_split("ds", "resnet50", "avg_pool") == "/data_root/ds/original/features/cnn_resnet50_avg_pool/"
    finally:
        configs.set_roots("../data", "../results")


def _write_maps(d, maps):
    os.makedirs(d, exist_ok=True)
    for i, m in enumerate(maps):
        np.save(os.path.join(d, "%d.npy" % i), m)


def test_load_feature_maps_no_normalisation(tmp_path):
    rs = np.random.RandomState(0)
    maps = (rs.standard_normal((5, 1, 2, 3, 8)) * 7).astype(np.float32)
    d = str(tmp_path / "cnn")
    _write_maps(d, maps)
    t, shape = models.load_acf_features(d + "/", 5, chunk=2)
    assert shape == (1, 2, 3, 8) and t.dtype == torch.float32
    np.testing.assert_array_equal(t.numpy(), maps.reshape(5, 6, 8))
    tb, _ = models.load_acf_features(d + "/", 5, dtype="bf16", chunk=3)
    assert tb.dtype == torch.bfloat16
    np.testing.assert_array_equal(tb.float().numpy(), torch.as_tensor(maps.reshape(5, 6, 8)).bfloat16().float().numpy())


def test_load_feature_maps_rejects_bad_shapes(tmp_path):
    rs = np.random.RandomState(1)
    d = str(tmp_path / "a")
    _write_maps(d, [rs.rand(1, 2, 2, 4).astype(np.float32), rs.rand(1, 2, 2, 5).astype(np.float32)])
    with pytest.raises(ValueError, match=r"1\.npy.*\(1, 2, 2, 5\)"):
        models.load_acf_features(d + "/", 2)
    d = str(tmp_path / "b")
    _write_maps(d, [rs.rand(2, 2, 4).astype(np.float32)])
    with pytest.raises(ValueError, match=r"0\.npy.*\(2, 2, 4\)"):
        models.load_acf_features(d + "/", 1)
    d = str(tmp_path / "c")
    _write_maps(d, [rs.rand(1, 2, 2, 4).astype(np.float32)])
    with pytest.raises(ValueError, match=r"1\.npy is missing"):
        models.load_acf_features(d + "/", 2)


class _StubEngine:
    def __init__(self, **kw):
        self.kw = kw

    def bind_acf(self, Gu, Gi, Bi, F, Pi, weights, train_lists, eval_lists=None, slots=None):
        self.bound = dict(Gu=Gu, Gi=Gi, Bi=Bi, F=F, Pi=Pi, weights=weights, train=train_lists, eval=eval_lists)
        return self


def _model(monkeypatch, validation=True, **over):
    monkeypatch.setattr(models, "Engine", _StubEngine)
    U, I = 30, 40
    rs = np.random.RandomState(4)
    train = [sorted(rs.choice(I, 5, replace=False).tolist()) for _ in range(U)]
    val = [[int(rs.randint(I))] for _ in range(U)] if validation else []
    data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=val, test_list=val,
                     params=Namespace(batch_eval=128))
    p = dict(epochs=1, batch_size=256, embed_k=128, lr=0.001, reg=0, top_k=20, dataset="toy", rec="acf",
             layers_component=[64, 1], layers_item=[64, 1], optimizer="adam_tf23", dtype="fp32", init_seed=0)
    p.update(over)
    F = np.abs(rs.standard_normal((I, 49, 512))).astype(np.float32)
    return models.ACF(data, Namespace(**p), features=F), data, F


def test_directory_parameters_match_the_reference(monkeypatch):
    m, _, _ = _model(monkeypatch)
    # ACF.py:46-51 with the reference's defaults
    assert m.directory_parameters == "batch_256-K_128-lr_0.001-reg_0-comp_[64, 1]-item_[64, 1]"
    m, _, _ = _model(monkeypatch, reg=0.5, layers_component=[32, 1], layers_item=[16, 1])
    assert m.directory_parameters == "batch_256-K_128-lr_0.001-reg_0.5-comp_[32, 1]-item_[16, 1]"


def test_creation_order_and_init(monkeypatch):
    m, data, F = _model(monkeypatch)
    b = m.engine.bound
    U, I, k, C, h, a = 30, 40, 128, 512, 64, 64
    rs = np.random.RandomState(0)
    lim = lambda r, c: np.sqrt(6.0 / (r + c))
    # BPRMF.py:48-50, then Pi (ACF.py:54), then the attention tensors in build_attention_weights' order
    np.testing.assert_array_equal(b["Gu"], rs.uniform(-lim(U, k), lim(U, k), (U, k)).astype(np.float32))
    np.testing.assert_array_equal(b["Gi"], rs.uniform(-lim(I, k), lim(I, k), (I, k)).astype(np.float32))
    np.testing.assert_array_equal(b["Pi"], rs.normal(0, 0.01, (I, k)).astype(np.float32))
    shapes = [("component.W_0_u", (k, h)), ("component.W_0_i", (C, h)), ("component.b_0", (h,)), ("component.W_1", (1, h)),
              ("component.b_1", (1,)), ("item.W_0_u", (k, a)), ("item.W_0_iv", (k, a)), ("item.W_0_ip", (k, a)),
              ("item.W_0_ix", (C, a)), ("item.b_0", (a,)), ("item.W_1", (1, a)), ("item.b_1", (1,))]
    assert [n for n, _ in shapes] == list(_ffi.ACF_WEIGHTS)
    for n, s in shapes:
        fi, fo = (s[0], s[1]) if len(s) == 2 else (s[0], s[0])      # TF's fan rule: 1-D shapes have fan_in = fan_out = n
        np.testing.assert_array_equal(b["weights"][n], rs.uniform(-lim(fi, fo), lim(fi, fo), s).astype(np.float32), err_msg=n)
    assert not np.any(b["Bi"])
    np.testing.assert_array_equal(b["F"].numpy(), F)                # not normalised
    assert b["eval"] == [tr + va for tr, va in zip(data.training_list, data.validation_list)]    # ACF.py:220
    assert b["train"] is data.training_list
    m, data, _ = _model(monkeypatch, validation=False)
    assert m.engine.bound["eval"] == data.training_list


def test_ref_gradient_is_detached():
    rs = np.random.RandomState(2)
    U, I, M, C, k = 6, 9, 4, 8, 5
    t = random_tables(rs, U, I, k, C, 3, 4, scale=10.0)
    F = np.abs(rs.standard_normal((I, M, C)))
    lists = [sorted(rs.choice(I, n, replace=False).tolist()) for n in (0, 1, 2, 3, 4, 5)]
    batch = ([0, 3, 3, 5], [1, 2, 2, 8], [4, 4, 7, 0])
    ref = ACFRef(t, F, reg=0.0)
    _, g = ref.grads(batch, lists)
    for n in ("Gu", "Pi") + tuple(_ffi.ACF_WEIGHTS):
        assert not torch.any(g[n]), n
    assert torch.any(g["Gi"])
    # the Gi gradient is the BPRMF item gradient with g'_u in place of gamma_u
    gp = ref.profiles(batch[0], lists)
    d = ((gp * ref.p["Gi"][batch[1]]).sum(1) - (gp * ref.p["Gi"][batch[2]]).sum(1))
    s = -torch.sigmoid(-d).unsqueeze(1) * gp
    want = torch.zeros_like(ref.p["Gi"]).index_add_(0, torch.tensor(batch[1]), s).index_add_(0, torch.tensor(batch[2]), -s)
    torch.testing.assert_close(g["Gi"], want, rtol=1e-12, atol=1e-14)
    # with reg > 0 every tensor moves by its own 2 reg w (and Gu / Pi per batch occurrence)
    ref = ACFRef(t, F, reg=0.3)
    _, g = ref.grads(batch, lists)
    for n in _ffi.ACF_WEIGHTS:
        torch.testing.assert_close(g[n], 0.6 * ref.p[n])
    want_gu = torch.zeros_like(ref.p["Gu"]).index_add_(0, torch.tensor(batch[0]), 0.6 * ref.p["Gu"][batch[0]])
    torch.testing.assert_close(g["Gu"], want_gu)


def test_ref_empty_history_is_the_user_row():
    rs = np.random.RandomState(3)
    t = random_tables(rs, 3, 5, 4, 6, 3, 3)
    ref = ACFRef(t, np.ones((5, 2, 6)))
    torch.testing.assert_close(ref.profile(1, []), ref.p["Gu"][1])
