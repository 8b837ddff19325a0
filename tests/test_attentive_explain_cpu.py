"""AttentiveFashion's explanation read-out without a GPU: the float64 restatement (tests/attentive_explain_ref.py) splits
AttentiveRef.call's score exactly over the three modalities and its edges share exactly over every grid; the new symbol is declared,
bound and exported; the CLI flag parses, is bounded and belongs to --rec attentive_fashion; the writer's row format on a stubbed
engine."""
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import attentive_explain_ref as X
from attentive_ref import AttentiveRef, random_inputs, random_tables
from fashionvisualexpl_recommend_amd import _ffi, evaluator, models, train_rec

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bprx.h")
REL = 1e-12


@pytest.fixture(scope="module")
def case():
    rs = np.random.RandomState(5)
    U, I, Dc, Dk, k = 4, 4, 9, 5, 6
    t = random_tables(rs, U, I, k, Dc, Dk, 8)
    inputs = random_inputs(rs, I, Dc, Dk)
    users, items = [0, 1, 2, 3, 1], [0, 1, 2, 3, 2]
    fine = X.explain(t, inputs, users, items, 112)
    return t, inputs, users, items, fine


def test_parts_sum_to_the_score_of_the_model(case):
    t, inputs, users, items, fine = case
    with torch.no_grad():
        x, alpha, _ = AttentiveRef(t, *inputs).call(users, items)
    scale = np.abs(fine["parts"]).sum(1)
    assert (np.abs(fine["parts"].sum(1) - x.numpy()) <= REL * scale).all()
    assert np.array_equal(fine["alpha"], alpha.numpy()) and np.array_equal(fine["score"], x.numpy())


def test_cells_sum_to_the_edges_share_and_rebin_for_every_grid(case):
    t, inputs, users, items, fine = case
    S = torch.as_tensor(fine["windows"])
    scale = np.abs(fine["windows"]).sum((1, 2))
    assert scale.min() > 0
    for G in X.GRIDS:
        m = X.explain(t, inputs, users, items, G)
        assert m["map"].shape == (len(users), G * G)
        assert (np.abs(m["map"].sum(1) - m["parts"][:, 1]) <= REL * scale).all(), G
        assert (np.abs(m["map"] - X.rebin(S, G).numpy()) <= REL * scale[:, None]).all(), G
        assert np.array_equal(m["peak_val"], m["map"].max(1))
        assert np.array_equal(m["parts"], fine["parts"])


def test_cell_order_is_row_major():
    S = torch.zeros((1, 112, 112), dtype=torch.float64)
    S[0, 3, 100] = 1.0                                               # window row 3, column 100
    assert int(X.rebin(S, 14).argmax()) == 0 * 14 + 12 and int(X.rebin(S, 112).argmax()) == 3 * 112 + 100
    assert int(X.rebin(S, 7).argmax()) == 6 and int(X.rebin(S, 16).argmax()) == 14


def test_float32_twin_is_the_same_code_and_close(case):
    t, inputs, users, items, _ = case
    r64 = X.explain(t, inputs, users, items, 14)
    r32 = X.explain(t, inputs, users, items, 14, dtype=torch.float32)
    allow = X.allowances(r64, r32)
    assert set(allow) == set(X.FIELDS)
    for n in X.FIELDS:
        assert 0.0 < allow[n] <= X.TOL_MULT * 1e-6, (n, allow[n])    # float32 rounding, not another formula


def test_symbol_in_header_binding_and_library():
    text = open(HEADER).read()
    assert "bprx_af_explain" in _ffi.EXPORTS
    assert "BPRX_API int bprx_af_explain(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, int32_t grid" in text
    assert _ffi.ABI_VERSION == 6 and "#define BPRX_ABI_VERSION 6" in text
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    assert hasattr(lib, "bprx_af_explain")


def test_cli_flag_default_values_and_model():
    assert train_rec.parse_args(["--rec", "attentive_fashion"]).af_explain == 0
    assert train_rec.parse_args(["--rec", "vbpr"]).af_explain == 0
    assert train_rec.parse_args(["--rec", "vbpr", "--af_explain", "0"]).af_explain == 0
    for ok in (1, 2, 4, 7, 8, 14, 16):
        assert train_rec.parse_args(["--rec", "attentive_fashion", "--af_explain", str(ok)]).af_explain == ok
    for bad in ("3", "-1", "28", "56", "112", "224"):
        with pytest.raises(SystemExit):
            train_rec.parse_args(["--rec", "attentive_fashion", "--af_explain", bad])
    for rec in ("bprmf", "vbpr", "grad_fashion", "acf"):
        with pytest.raises(SystemExit):
            train_rec.parse_args(["--rec", rec, "--af_explain", "7"])


class _StubEngine:
    def __init__(self, **kw):
        self.kw = kw

    def bind_attentive(self, *a, **kw):
        return self


def test_directory_parameters_do_not_change_with_the_flag(monkeypatch):
    monkeypatch.setattr(models, "Engine", _StubEngine)
    U, I = 6, 5
    rs = np.random.RandomState(4)
    train = [sorted(rs.choice(I, 2, replace=False).tolist()) for _ in range(U)]
    data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=[], test_list=[],
                     params=Namespace(batch_eval=128))
    p = dict(epochs=1, batch_size=256, embed_k=16, lr=0.001, reg=0, top_k=20, dataset="toy", rec="attentive_fashion",
             attention_layers=[64, 1], dropout=0.5, optimizer="adam_tf23", dtype="fp32", init_seed=0)
    inputs = (np.zeros((I, 224, 224), np.uint8), np.ones((I, 3), np.float32), np.ones((I, 2), np.float32))
    plain = models.AttentiveFashion(data, Namespace(**p), inputs=inputs)
    assert plain.af_explain == 0
    m = models.AttentiveFashion(data, Namespace(af_explain=7, **p), inputs=inputs)
    assert m.af_explain == 7 and m.directory_parameters == plain.directory_parameters
    with pytest.raises(ValueError, match="af_explain"):
        models.AttentiveFashion(data, Namespace(af_explain=3, **p), inputs=inputs)


class _ExplainStub:
    """af_explain of three fixed pairs at G = 2."""
    def af_explain(self, users, items, grid, maps=True):
        assert grid == 2 and maps and list(users) == [0, 0, 3] and list(items) == [5, 2, 7]
        f = lambda a: torch.tensor(a, dtype=torch.float32)
        return {"score": f([1.5, -0.25, 0.0]), "alpha": f([[0.5, 0.25, 0.25]] * 3),
                "parts": f([[1.0, 0.25, 0.25], [-0.5, 0.125, 0.125], [0.0, 0.0, 0.0]]),
                "peak_cell": torch.tensor([3, 0, 1], dtype=torch.int32), "peak_val": f([0.5, 0.0625, 0.0]),
                "map": f([[0.0, -0.125, -0.125, 0.5], [0.0625, 0.0625, 0.0, 0.0], [-1.0, 0.0, 0.0, -2.0]])}


def test_writer_row_format_on_a_stubbed_engine(tmp_path, monkeypatch):
    ev = evaluator.Evaluator.__new__(evaluator.Evaluator)
    ev.model = Namespace(engine=_ExplainStub())

    def rows(self, out, block_hook=None):
        out.write("0\t5\t1.5\t0.5\t0.25\t0.25\n0\t2\t-0.25\t0.5\t0.25\t0.25\n")
        out.write("3\t7\t0.0\t0.5\t0.25\t0.25\n")
        block_hook([0, 0, 3], [5, 2, 7])
    monkeypatch.setattr(evaluator.Evaluator, "_store_attention_rows", rows)
    recs, expl = str(tmp_path / "recs.tsv"), str(tmp_path / "expl.tsv")
    ev.store_recommendation_attention_explain(recs, expl, 2)
    assert len(open(recs).read().splitlines()) == 3
    got = [l.split("\t") for l in open(expl).read().splitlines()]
    assert got == [
        ["0", "5", "1.5", "1.0", "0.25", "0.25", "1", "1", "0.5", "0.0", "-0.125", "-0.125", "0.5"],
        ["0", "2", "-0.25", "-0.5", "0.125", "0.125", "0", "0", "0.0625", "0.0625", "0.0625", "0.0", "0.0"],
        ["3", "7", "0.0", "0.0", "0.0", "0.0", "0", "1", "0.0", "-1.0", "0.0", "0.0", "-2.0"]]
    assert all(len(r) == 9 + 4 for r in got)
