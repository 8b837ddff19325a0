"""AttentiveFashion without a GPU: the CLI flags and rejections, the three loaders, directory_parameters, creation order and
initialiser ranges on a stub engine, the sanity of the float64 restatement (tests/attentive_ref.py) and the ABI exports."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from attentive_ref import AF_WEIGHTS, AttentiveRef, random_inputs, random_tables
from fashionvisualexpl_recommend_amd import _ffi, configs, models, synth, train_rec


def test_cli_flags_and_defaults():
    a = train_rec.parse_args(["--rec", "attentive_fashion"])
    assert (a.rec, a.attention_layers, a.dropout, a.dtype, a.optimizer) == ("attentive_fashion", [64, 1], 0.5, "fp32", "adam_tf23")
    a = train_rec.parse_args(["--rec", "attentive_fashion", "--attention_layers", "32", "1", "--dropout", "0", "--optimizer", "sgd"])
    assert (a.attention_layers, a.dropout, a.optimizer) == ([32, 1], 0.0, "sgd")
    assert train_rec.parse_args([]).rec == "vbpr"                    # the default model stays what it was


@pytest.mark.parametrize("bad", [["64"], ["64", "2"], ["64", "1", "1"], ["0", "1"]])
def test_cli_rejects_other_layer_forms(bad):
    with pytest.raises(SystemExit):
        train_rec.parse_args(["--rec", "attentive_fashion", "--attention_layers"] + bad)


def test_cli_rejects_bad_dropout_multi_gpu_and_other_dtypes():
    with pytest.raises(SystemExit):
        train_rec.parse_args(["--rec", "attentive_fashion", "--dropout", "1.0"])
    with pytest.raises(NotImplementedError, match="attentive_fashion"):
        train_rec.train(["--rec", "attentive_fashion", "--world_size", "2"])
    with pytest.raises(ValueError, match="fp32"):
        train_rec.train(["--rec", "attentive_fashion", "--dtype", "bf16"])


def test_input_paths():
    configs.set_roots("/data_root", "/res_root")
    try:
        assert configs.edges_path("ds") == "/data_root/ds/original/features/edges/"
        assert configs.hist_color_features_path_dir("ds") == "/data_root/ds/original/features/color_histograms/"
        assert configs.class_features_path_dir("ds") == "/data_root/ds/original/features/one_hot_encodings/"
    finally:
        configs.set_roots("../data", "../results")


def test_loaders(tmp_path):
    from PIL import Image
    root = str(tmp_path)
    edges, color, cls = synth.write_attentive_features(root, "toy", 6, dim_color=13, dim_class=5, image_size=40)
    assert edges.shape == (6, 40, 40) and not edges[0].any() and edges[1:].any()
    configs.set_roots(root, root)
    try:
        e, c, k = models.load_attentive_inputs("toy", 6)
        assert e.dtype == torch.uint8 and tuple(e.shape) == (6, 224, 224) and c.dtype == torch.float32 and tuple(c.shape) == (6, 13)
        for i in range(6):                                           # the resize is PIL's own (dataset.py:172)
            want = np.array(Image.open(os.path.join(root, "toy/original/features/edges/%d.tiff" % i)).convert('L').resize((224, 224)))
            np.testing.assert_array_equal(e[i].numpy(), want)
            np.testing.assert_array_equal(c[i].numpy(), (color[i] / np.max(np.abs(color[i]))).astype(np.float32))
        assert float(c.abs().max(1).values.min()) == 1.0             # every histogram by its OWN max-abs
        np.testing.assert_array_equal(k.numpy(), cls)
        d = os.path.join(root, "toy/original/features/")
        np.save(d + "color_histograms/4.npy", np.zeros(13, np.float32))
        with pytest.raises(ValueError, match=r"color_histograms/4\.npy is all zero"):
            models.load_attentive_inputs("toy", 6)
        os.remove(d + "one_hot_encodings/2.npy")
        with pytest.raises(ValueError, match=r"one_hot_encodings/2\.npy is missing"):
            models.load_attentive_inputs("toy", 6)
    finally:
        configs.set_roots("../data", "../results")


class _StubEngine:
    def __init__(self, **kw):
        self.kw = kw

    def bind_attentive(self, Gu, Gi, Bi, edges, color, cls, weights, dropout=0.5, seed=0, slots=None):
        self.bound = dict(Gu=Gu, Gi=Gi, Bi=Bi, edges=edges, color=color, cls=cls, weights=weights, dropout=dropout, seed=seed)
        return self


def _model(monkeypatch, **over):
    monkeypatch.setattr(models, "Engine", _StubEngine)
    U, I, Dc, Dk = 30, 12, 24, 10
    rs = np.random.RandomState(4)
    train = [sorted(rs.choice(I, 5, replace=False).tolist()) for _ in range(U)]
    val = [[int(rs.randint(I))] for _ in range(U)]
    data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=val, test_list=val, params=Namespace(batch_eval=128))
    p = dict(epochs=1, batch_size=256, embed_k=128, lr=0.001, reg=0, top_k=20, dataset="toy", rec="attentive_fashion",
             attention_layers=[64, 1], dropout=0.5, optimizer="adam_tf23", dtype="fp32", init_seed=0)
    p.update(over)
    inputs = (np.zeros((I, 224, 224), np.uint8), rs.rand(I, Dc).astype(np.float32), rs.rand(I, Dk).astype(np.float32))
    return models.AttentiveFashion(data, Namespace(**p), inputs=inputs)


def test_directory_parameters_match_the_reference(monkeypatch):
    # AttentiveFashion.py:275-279 with the reference's defaults
    assert _model(monkeypatch).directory_parameters == "batch_256-K_128-lr_0.001-reg_0-attlayers_[64, 1]"
    assert _model(monkeypatch, reg=0.5, attention_layers=[32, 1]).directory_parameters.endswith("-reg_0.5-attlayers_[32, 1]")
    with pytest.raises(ValueError, match="attention_layers"):
        _model(monkeypatch, attention_layers=[64, 2])
    with pytest.raises(ValueError, match="fp32"):
        _model(monkeypatch, dtype="bf16")


def test_creation_order_and_init(monkeypatch):
    m = _model(monkeypatch)
    b = m.engine.bound
    U, I, k, Dc, Dk, h = 30, 12, 128, 24, 10, 64
    rs = np.random.RandomState(0)
    lim = lambda r, c: np.sqrt(6.0 / (r + c))
    uni = lambda r, c, s: rs.uniform(-lim(r, c), lim(r, c), s).astype(np.float32)
    # BPRMF.py:48-50 (Glorot: the RandomNormal of AttentiveFashion.py:24 is assigned after the tables exist and is never read), then
    # the colour, edges and class encoders, then the attention tensors
    np.testing.assert_array_equal(b["Gu"], uni(U, k, (U, k)))
    np.testing.assert_array_equal(b["Gi"], uni(I, k, (I, k)))
    assert not np.any(b["Bi"])
    w = b["weights"]
    assert list(w) == list(_ffi.AF_WEIGHTS) == list(AF_WEIGHTS)
    np.testing.assert_array_equal(w["color.W1"], uni(Dc, 256, (Dc, 256)))
    np.testing.assert_array_equal(w["color.W2"], uni(256, k, (256, k)))
    np.testing.assert_array_equal(w["edges.conv"], uni(25, 25 * 64, (25, 64)))       # Conv2D fans: 5*5*1 and 5*5*64
    np.testing.assert_array_equal(w["edges.W2"], uni(64, k, (64, k)))
    np.testing.assert_array_equal(w["class.W1"], uni(Dk, 256, (Dk, 256)))
    np.testing.assert_array_equal(w["class.W2"], uni(256, k, (256, k)))
    np.testing.assert_array_equal(w["attention.W_1"], uni(k, h, (k, h)))
    np.testing.assert_array_equal(w["attention.b_1"], uni(h, h, h))
    np.testing.assert_array_equal(w["attention.W_2"], uni(h, 1, (h, 1)))
    np.testing.assert_array_equal(w["attention.b_2"], uni(1, 1, 1))
    for n in ("color.b1", "edges.conv_b", "class.b1"):               # Keras biases start at zero
        assert not np.any(w[n])
    assert np.abs(w["edges.conv"]).max() <= np.sqrt(6.0 / 1625)
    assert b["dropout"] == 0.5


def _small(seed=2, U=5, I=4, k=8, Dc=7, Dk=3, h=16):
    rs = np.random.RandomState(seed)
    t = random_tables(rs, U, I, k, Dc, Dk, h)
    return rs, t, random_inputs(rs, I, Dc, Dk)


def test_ref_attention_sums_to_one_in_colour_edges_class_order():
    rs, t, inputs = _small()
    ref = AttentiveRef(t, *inputs)
    with torch.no_grad():
        x, alpha, enc = ref.call([0, 1, 4], [0, 1, 3])
        assert alpha.shape == (3, 3) and (alpha.sum(1) - 1).abs().max().item() <= 1e-12
        # component 1 is the edge encoder: a blank image (item 0) with zero conv bias encodes to zero
        ref.p["edges.conv_b"].zero_()
        assert ref.encode(ref.p, [0])[1].abs().max().item() == 0.0
        assert ref.encode(ref.p, [0])[0].abs().max().item() > 0.0
        # the score is the attention-weighted sum of the three per-component scores
        gu, gi = ref.p["Gu"][[0, 1, 4]], ref.p["Gi"][[0, 1, 3]]
        enc = ref.encode(ref.p, [0, 1, 3])
        x, alpha = ref.score(ref.p, gu, gi, enc)
        want = sum(alpha[:, l] * (gu * enc[l] * gi).sum(1) for l in range(3))
        assert (x - want).abs().max().item() <= 1e-12


def test_ref_rate_zero_is_deterministic_and_nothing_is_detached():
    rs, t, inputs = _small()
    batch = ([0, 1, 2], [1, 2, 3], [3, 3, 1])
    a = AttentiveRef(t, *inputs, reg=0.1, rate=0.0)
    b = AttentiveRef(t, *inputs, reg=0.1, rate=0.0)
    ones = (torch.ones(6, 256), torch.ones(6, 64), torch.ones(6, 256))
    la, ga = a.grads(batch, None)
    lb, gb = b.grads(batch, ones)                                    # rate 0: an all-ones mask with scale 1 is no mask
    assert la == lb and all(torch.equal(ga[n], gb[n]) for n in ga)
    for n in ("Gu", "Gi") + tuple(AF_WEIGHTS):                       # the gradient reaches every tensor, the conv kernel included
        assert ga[n].abs().max().item() > 0.0, n
    # a dropped unit carries no gradient
    masks = (torch.zeros(6, 256), torch.ones(6, 64), torch.ones(6, 256))
    _, g = AttentiveRef(t, *inputs, reg=0.0, rate=0.5).grads(batch, masks)
    assert g["color.W1"].abs().max().item() == 0.0 and g["class.W1"].abs().max().item() > 0.0


def test_ref_adam_rules():
    rs, t, inputs = _small()
    ref = AttentiveRef(t, *inputs, reg=0.1, rate=0.0)
    before = {n: v.clone() for n, v in ref.p.items()}
    ref.step(([0, 1], [1, 2], [3, 0]), None, "adam_tf23", 1e-3)
    # first Adam step: |update| = lr_t * (1-b1)|g| / (sqrt((1-b2) g^2) + eps) ~ lr wherever g != 0; TF's sparse rule moves only
    # rows with a gradient at step 1 (m = v = 0 elsewhere)
    d = (ref.p["Gu"] - before["Gu"]).abs()
    assert d[[0, 1]].max().item() == pytest.approx(1e-3, rel=1e-3) and d[[2, 3, 4]].max().item() == 0.0


def test_abi_exports_the_new_symbols():
    for sym in ("bprx_bind_attentive", "bprx_af_encode", "bprx_af_attention_pairs", "bprx_af_score_block", "bprx_af_dropout_mask",
                "bprx_af_get_step", "bprx_af_set_step"):
        assert sym in _ffi.EXPORTS
    lib = _ffi.lib()
    assert lib.bprx_abi_version() == _ffi.ABI_VERSION == 6
    assert all(hasattr(lib, s) for s in _ffi.EXPORTS)
    assert _ffi.Attentive.w.size == 13 * 8 and len(_ffi.AF_WEIGHTS) == 13
