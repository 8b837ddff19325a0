"""bprx_feat_explain without a GPU: the identities of the float64 restatement (tests/feat_explain_ref.py) -- the map sums to the
visual part, base + visual is the VBPR score of tests/torch_ref.py and the GradFashion score of tests/gradfashion_ref.py, the colour
and edge column ranges sum to predict_ui_grads --, the tie rule of its list, the new symbol (declared, bound, exported, ABI still 6)
and the rules of --feat_explain."""
import os
import re

import numpy as np
import pytest
import torch

import feat_explain_ref as X
import torch_ref
from fashionvisualexpl_recommend_amd import _ffi, train_rec
from gradfashion_ref import GradFashionRef

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bprx.h")


def _dyadic_tables(U=30, I=50, k=8, d=6, D=40, seed=0):
    """F in multiples of 1/8, E and Bp in multiples of 1/16, all of magnitude <= 1: bf16 holds them exactly and every product
    and partial sum of F [E|Bp] is a multiple of 1/128 below 2^6, exact in float32 in any order.  torch_ref.vbpr_forward (bf16
    operand, float32 matmul) is then an exact projection, and its score with float64 row tables a float64 VBPR score."""
    rs = np.random.RandomState(seed)
    q = lambda n, *shape: torch.as_tensor(rs.randint(-n, n + 1, size=shape) / float(n), dtype=torch.float64)
    g = lambda *shape: torch.as_tensor(rs.standard_normal(shape) * 0.3, dtype=torch.float64)
    return dict(Gu=g(U, k), Gi=g(I, k), Bi=g(I), Tu=g(U, d), F=q(8, I, D).abs().float(), E=q(16, D, d), Bp=q(16, D))


def test_map_sums_to_visual_and_base_plus_visual_is_the_vbpr_score():
    t = _dyadic_tables()
    rs = np.random.RandomState(1)
    u, i = rs.randint(30, size=200), rs.randint(50, size=200)
    for ncols in (40, 33):
        tt = dict(t)
        if ncols < 40:                                             # the columns beyond ncols are the models' zero padding
            tt["F"] = t["F"].clone()
            tt["F"][:, ncols:] = 0
        r = X.feat_explain_ref(tt, u, i, ncols)
        assert r["map"].shape == (200, ncols) and r["map"].dtype == np.float64
        np.testing.assert_allclose(r["map"].sum(1), r["visual"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(r["base"] + r["visual"], r["score"], rtol=0, atol=1e-12)
        state = dict(tt, F=tt["F"].float())
        ui, ii = torch.as_tensor(u), torch.as_tensor(i)
        fwd = torch_ref.vbpr_forward(state, (ui, ii, ii), fp8=False)
        assert fwd["xp"].dtype == torch.float64
        np.testing.assert_allclose(r["score"], fwd["xp"].numpy(), rtol=0, atol=1e-12)
    r64, r32 = X.feat_explain_ref(t, u, i, 40), X.feat_explain_ref(t, u, i, 40, torch.float32)
    assert r32["map"].dtype == np.float32 and 0 < np.abs(r32["score"] - r64["score"]).max() < 1e-5


def test_factored_model_colour_and_edge_ranges_sum_to_predict_ui_grads():
    rs = np.random.RandomState(2)
    U, I, k, d, Dc, De, ec, ee = 20, 30, 8, 6, 10, 22, 4, 5
    g = lambda *s: rs.standard_normal(s) * 0.3
    t = dict(Gu=g(U, k), Gi=g(I, k), Bi=g(I), Tu=g(U, d), Fc=np.abs(g(I, Dc)), Fe=np.abs(g(I, De)), Ec=g(Dc, ec), Ee=g(De, ee),
             E=g(ec + ee, d), Bp=g(ec + ee))
    ref = GradFashionRef(t, reg=0.0)
    E_eff, Bp_eff = ref.effective()
    F = np.zeros((I, 48))                                           # [Fc | Fe | zero padding]
    F[:, :Dc], F[:, Dc:Dc + De] = t["Fc"], t["Fe"]
    tt = dict(Gu=t["Gu"], Gi=t["Gi"], Bi=t["Bi"], Tu=t["Tu"], F=F, E=torch.cat([E_eff, torch.zeros(48 - Dc - De, d, dtype=torch.float64)]),
              Bp=torch.cat([Bp_eff, torch.zeros(48 - Dc - De, dtype=torch.float64)]))
    u, i = rs.randint(U, size=60), rs.randint(I, size=60)
    r = X.feat_explain_ref(tt, u, i, Dc + De)
    np.testing.assert_allclose(r["score"], ref.call(u, i)[0].numpy(), rtol=0, atol=1e-12)
    want = np.concatenate([ref.predict_ui_grads(int(a), int(b)) for a, b in zip(u, i)])
    np.testing.assert_allclose(r["map"][:, :Dc].sum(1), want[:, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["map"][:, Dc:].sum(1), want[:, 1], rtol=0, atol=1e-12)


def test_list_rule_of_the_restatement():
    row = np.array([0.5, -0.0, 2.0, 0.0, 2.0, -1.0, 0.0], np.float32)
    cols, vals = X.top_columns(row, 5)
    assert cols.tolist() == [2, 4, 0, 1, 3] and vals.tolist() == [2.0, 2.0, 0.5, 0.0, 0.0]
    assert X.top_columns(row, 32)[0].tolist() == [2, 4, 0, 1, 3, 6, 5]


def test_symbol_is_declared_bound_and_exported():
    hdr = open(HEADER).read()
    assert re.search(r"BPRX_API\s+int\s+bprx_feat_explain\s*\(", hdr)
    assert re.search(r"#define\s+BPRX_ABI_VERSION\s+6\b", hdr)
    assert "bprx_feat_explain" in _ffi.EXPORTS and _ffi.ABI_VERSION == 6
    fn = _ffi.lib().bprx_feat_explain
    assert len(fn.argtypes) == 14 and _ffi.lib().bprx_abi_version() == 6
    assert fn(None, None, None, None, 0, 1, 1, None, None, None, None, None, None, None) == _ffi.E_INVALID      # no handle


def test_cli_flag_default_bounds_and_models():
    assert train_rec.parse_args(["--rec", "vbpr"]).feat_explain == 0
    assert train_rec.parse_args(["--rec", "acf"]).feat_explain == 0
    assert train_rec.parse_args(["--rec", "vbpr", "--feat_explain", "3"]).feat_explain == 3
    assert train_rec.parse_args(["--rec", "grad_fashion", "--feat_explain", "32"]).feat_explain == 32
    assert train_rec.parse_args(["--rec", "bprmf", "--feat_explain", "0"]).feat_explain == 0
    for bad in ("33", "-1"):
        with pytest.raises(SystemExit):
            train_rec.parse_args(["--rec", "vbpr", "--feat_explain", bad])
    for rec in ("bprmf", "acf", "attentive_fashion"):
        with pytest.raises(SystemExit):
            train_rec.parse_args(["--rec", rec, "--feat_explain", "3"])
    for rec in ("vbpr", "grad_fashion"):                            # the sharded drivers write no expl-* files
        with pytest.raises(NotImplementedError):
            train_rec.train(["--rec", rec, "--feat_explain", "3", "--world_size", "2"])
