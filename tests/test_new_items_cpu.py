"""New-item scoring without a GPU: the float32 restatement (tests/new_items_ref.py) against the float64 one, the five new symbols
(declared, bound, exported, ABI still 6; a NULL handle is rejected), the rules of --new_items, and the normalisation helper."""
import os
import re

import numpy as np
import pytest
import torch

import new_items_ref as N
from fashionvisualexpl_recommend_amd import _ffi, train_rec
from fashionvisualexpl_recommend_amd.models import normalize_new_rows

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bprx.h")
SYMBOLS = {"bprx_proj_stride": 1, "bprx_project_rows": 5, "bprx_score_new_block": 7, "bprx_topk_rows": 9, "bprx_feat_explain_new": 13}


def _tables(n=40, D=128, d=12, U=30, seed=0):
    rs = np.random.RandomState(seed)
    F = np.abs(rs.standard_normal((n, D))).astype(np.float32)
    return dict(F=F / F.max(), E=(rs.standard_normal((D, d)) * 0.2).astype(np.float32),
                Bp=(rs.standard_normal(D) * 0.2).astype(np.float32), Tu=(rs.standard_normal((U, d)) * 0.3).astype(np.float32))


@pytest.mark.parametrize("feat_dtype", ["fp32", "bf16"])
def test_float32_restatement_agrees_with_float64(feat_dtype):
    t = _tables()
    F = N.orc.bf16_round(t["F"]) if feat_dtype == "bf16" else t["F"]
    P64, P32 = (N.projection(F, t["E"], t["Bp"], feat_dtype, dt) for dt in (torch.float64, torch.float32))
    assert P64.shape == (40, 13) and P64.dtype == np.float64 and P32.dtype == np.float32
    assert 0 < np.abs(P64 - P32).max() < 1e-5
    S64, S32 = (N.scores(t["Tu"], F, t["E"], t["Bp"], 3, 30, feat_dtype, dt) for dt in (torch.float64, torch.float32))
    assert S64.shape == (27, 40) and 0 < np.abs(S64 - S32).max() < 1e-5
    rs = np.random.RandomState(1)
    u, r = rs.randint(30, size=60), rs.randint(40, size=60)
    e64, e32 = (N.explain(t["Tu"], F, t["E"], t["Bp"], u, r, 100, dt) for dt in (torch.float64, torch.float32))
    assert e64["map"].shape == (60, 100) and np.abs(e64["map"] - e32["map"]).max() < 1e-5
    assert np.abs(e64["score"] - e32["score"]).max() < 1e-5
    np.testing.assert_allclose(e64["map"].sum(1), e64["score"], rtol=0, atol=1e-12)
    if feat_dtype == "fp32":                    # all columns, master weights: the explanation's score is the score block's entry
        full = N.explain(t["Tu"], F, t["E"], t["Bp"], u, r, 128)["score"]
        np.testing.assert_allclose(full, N.scores(t["Tu"], F, t["E"], t["Bp"], 0, 30)[u, r], rtol=0, atol=1e-12)


def test_symbols_are_declared_bound_and_exported():
    hdr = open(HEADER).read()
    assert re.search(r"#define\s+BPRX_ABI_VERSION\s+6\b", hdr) and _ffi.ABI_VERSION == 6
    lib = _ffi.lib()
    assert lib.bprx_abi_version() == 6
    for name, nargs in SYMBOLS.items():
        assert re.search(r"BPRX_API\s+int(32_t)?\s+%s\s*\(" % name, hdr), name
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs, name


def test_a_null_handle_is_rejected():
    lib = _ffi.lib()
    assert lib.bprx_proj_stride(None) < 0
    assert lib.bprx_project_rows(None, None, 0, None, None) == _ffi.E_INVALID
    assert lib.bprx_score_new_block(None, 0, 0, None, 0, None, None) == _ffi.E_INVALID
    assert lib.bprx_topk_rows(None, 0, 1, None, 1, None, None, None, None) == _ffi.E_INVALID
    assert lib.bprx_feat_explain_new(None, None, 0, None, None, 0, 1, 1, None, None, None, None, None) == _ffi.E_INVALID


def test_cli_flag_paths_and_models():
    assert train_rec.parse_args(["--rec", "vbpr"]).new_items is None
    assert train_rec.parse_args(["--rec", "vbpr", "--new_items", "a.npy"]).new_items == ["a.npy"]
    assert train_rec.parse_args(["--rec", "grad_fashion", "--new_items", "c.npy", "e.npy"]).new_items == ["c.npy", "e.npy"]
    for argv in (["--rec", "acf", "--new_items", "a.npy"], ["--rec", "bprmf", "--new_items", "a.npy"],
                 ["--rec", "attentive_fashion", "--new_items", "a.npy"], ["--rec", "grad_fashion", "--new_items", "a.npy"],
                 ["--rec", "vbpr", "--new_items", "a.npy", "b.npy"]):
        with pytest.raises(SystemExit):
            train_rec.parse_args(argv)
    with pytest.raises(NotImplementedError):
        train_rec.train(["--rec", "vbpr", "--new_items", "a.npy", "--world_size", "2"])
    with pytest.raises(ValueError):
        train_rec.train(["--rec", "vbpr", "--new_items", "a.npy", "--dtype", "fp8"])


@pytest.mark.parametrize("file_dtype", [np.float64, np.float32])
def test_normalisation_gives_bit_equal_rows_for_equal_raw_rows(tmp_path, file_dtype):
    """What the models do with a training file (np.load, divide by the global max-abs, float32 table) against the helper on raw
    rows taken from the same file, through a snapshot of the divisor (a 0-dim tensor, as state_dict keeps it)."""
    rs = np.random.RandomState(2)
    raw = (rs.standard_normal((50, 24)) * 7.3).astype(file_dtype)
    np.save(str(tmp_path / "f.npy"), raw)
    f = np.load(str(tmp_path / "f.npy"))
    norm = np.max(np.abs(f))
    table = (f / norm).astype(np.float32)
    kept = torch.as_tensor(np.asarray(norm)).cpu().numpy()[()]
    assert kept.dtype == norm.dtype and kept == norm
    pick = [49, 0, 7, 7]
    new = normalize_new_rows(f[pick], kept, 24)
    assert new.dtype == np.float32 and new.shape == (4, 24)
    assert np.array_equal(new.view(np.uint32), table[pick].view(np.uint32))
    above = normalize_new_rows(f[:2] * 3, kept, 24)                 # a new row may exceed the training max-abs
    assert np.abs(above).max() <= 3.0 and np.isfinite(above).all()
    for bad in (f[:3, :20], f[0]):
        with pytest.raises(ValueError):
            normalize_new_rows(bad, kept, 24)
