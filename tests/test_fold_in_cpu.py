"""Folding in new users without a GPU: the restatement (tests/fold_in_ref.py) against the oracle's train step, the pair sampler,
the three new symbols (declared, bound, exported, ABI still 6; a NULL handle is rejected), and the rules of --new_users."""
import os
import re

import numpy as np
import pytest

import fold_in_ref as R
from fashionvisualexpl_recommend_amd import _ffi, synth, train_rec
from fashionvisualexpl_recommend_amd.models import draw_fold_pairs
from oracle import oracle as orc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bprx.h")
SYMBOLS = {"bprx_fold_in": 13, "bprx_score_rows_block": 8, "bprx_topk_lists": 10}
# what tests/test_oracle_step.py holds an oracle step to, per optimizer
STEP_TOL = {"sgd": dict(rtol=2e-6, atol=2e-7), "adam_tf23": dict(rtol=2e-4, atol=2e-6)}


def _tables(U, I, k, d=0, D=0, seed=0):
    rs = np.random.RandomState(seed)
    t = dict(Gu=synth.glorot_uniform(rs, U, k), Gi=synth.glorot_uniform(rs, I, k), Bi=(rs.standard_normal(I) * 0.1).astype(np.float32))
    if d:
        F = synth.make_features(I, D, seed=seed)
        t.update(Tu=synth.glorot_uniform(rs, U, d), F=(F / np.abs(F).max()).astype(np.float32), E=synth.glorot_uniform(rs, D, d),
                 Bp=synth.glorot_uniform(rs, D, 1).reshape(-1))
    return t


@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
@pytest.mark.parametrize("model", ["bprmf", "vbpr"])
def test_one_step_of_the_restatement_is_the_oracles_step_for_that_user(model, opt):
    """T = 1, the batch one user's pairs (duplicates and an i == j pair among them): the restatement moves the user's row as
    oracle.OracleModel.step moves Gu_u / Tu_u (adam_tf23 from zero slots)."""
    U, I, k = 12, 40, 8
    d, D = (6, 64) if model == "vbpr" else (0, 0)
    t = _tables(U, I, k, d, D, seed=3)
    rs = np.random.RandomState(4)
    u, B, lr, reg = 5, 23, 0.05, 1e-2
    pos, neg = rs.randint(I, size=B), rs.randint(I, size=B)
    pos[3], neg[3] = pos[2], neg[2]
    neg[7] = pos[7]
    m = orc.OracleModel(**t)
    m.step(np.full(B, u), pos, neg, opt, lr, reg)
    P = None
    if d:
        F64 = t["F"].astype(np.float64)
        P = np.concatenate([F64 @ t["E"], (F64 @ t["Bp"])[:, None]], 1).astype(np.float32)
    r = R.fold_in(t["Gi"], t["Bi"], P, [0, B], pos, neg, t["Gu"][u:u + 1], t["Tu"][u:u + 1] if d else None, 1, lr, reg, opt)
    np.testing.assert_allclose(m.Gu[u], r["Gu"][0], err_msg="Gu", **STEP_TOL[opt])
    assert np.abs(m.Gu[u] - t["Gu"][u]).max() > 1e-4                       # (the step moved the row at all)
    if d:
        np.testing.assert_allclose(m.Tu[u], r["Tu"][0], err_msg="Tu", **STEP_TOL[opt])
    others = np.arange(U) != u                                             # the other users' rows: regularised by nobody's pairs
    if opt == "sgd":
        assert np.array_equal(m.Gu[others], t["Gu"][others])


def test_float32_restatement_agrees_with_float64_and_keeps_empty_users():
    t = _tables(4, 50, 16, seed=5)
    rs = np.random.RandomState(6)
    ptr = [0, 7, 7, 12]
    pos, neg = rs.randint(50, size=12), rs.randint(50, size=12)
    G0 = (rs.standard_normal((3, 16)) * 0.3).astype(np.float32)
    for opt in ("sgd", "adam_tf23"):
        r64, r32 = (R.fold_in(t["Gi"], t["Bi"], None, ptr, pos, neg, G0, None, 5, 0.05, 1e-2, opt, dt) for dt in (np.float64, np.float32))
        assert r64["Gu"].dtype == np.float64 and r32["Gu"].dtype == np.float32 and r64["Tu"] is None
        assert 0 < np.abs(r64["Gu"] - r32["Gu"]).max() < 1e-5
        assert np.array_equal(r32["Gu"][1], G0[1]) and r64["loss"][1] == 0 and r64["grads"][1].shape == (0, 16)
        assert r64["grads"][0].shape == (5, 16) and (r64["loss"][[0, 2]] > 0).all()


def test_draw_fold_pairs():
    I = 30
    hist = [[3, 4, 5], [], list(range(I)), [7], [9, 9, 2]]
    ptr, pos, neg = draw_fold_pairs(hist, I, 4, seed=1)
    assert ptr.dtype == np.int64 and pos.dtype == np.int32 and neg.dtype == np.int32
    assert ptr.tolist() == [0, 12, 12, 12, 16, 28]                        # no pairs: an empty history, one that covers the catalogue
    for r, h in enumerate(hist):
        p, n = pos[ptr[r]:ptr[r + 1]], neg[ptr[r]:ptr[r + 1]]
        if len(p):
            assert p.tolist() == np.repeat(h, 4).tolist()                 # positives in history order, `negatives` draws each
        assert not set(n.tolist()) & set(h)
        assert ((n >= 0) & (n < I)).all()
    again = draw_fold_pairs(hist, I, 4, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip((ptr, pos, neg), again))
    assert not np.array_equal(draw_fold_pairs(hist, I, 4, seed=2)[2], neg)
    most = [[i for i in range(I) if i != 11]]                             # one item left: every negative is that item
    assert set(draw_fold_pairs(most, I, 2, seed=0)[2].tolist()) == {11}
    for bad in ([[0, I]], [[-1]]):
        with pytest.raises(ValueError):
            draw_fold_pairs(bad, I, 4, seed=0)
    e = draw_fold_pairs([], I, 4, seed=0)
    assert e[0].tolist() == [0] and e[1].size == 0 and e[2].size == 0


def test_symbols_are_declared_bound_and_exported():
    hdr = open(HEADER).read()
    assert re.search(r"#define\s+BPRX_ABI_VERSION\s+6\b", hdr) and _ffi.ABI_VERSION == 6
    lib = _ffi.lib()
    assert lib.bprx_abi_version() == 6
    for name, nargs in SYMBOLS.items():
        assert re.search(r"BPRX_API\s+int\s+%s\s*\(" % name, hdr), name
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs, name


def test_a_null_handle_is_rejected():
    lib = _ffi.lib()
    assert lib.bprx_fold_in(None, None, None, None, 0, 1, 0.1, 0.0, 0, None, None, None, None) == _ffi.E_INVALID
    assert lib.bprx_score_rows_block(None, None, None, 0, 0, 0, None, None) == _ffi.E_INVALID
    assert lib.bprx_topk_lists(None, 0, None, None, None, 1, None, None, None, None) == _ffi.E_INVALID


def test_new_users_file(tmp_path):
    p = tmp_path / "new.tsv"
    p.write_text("anna b\t5\nzed\t7\n\nanna b\t2\nzed\t7\n09\t1\n")
    labels, lists = train_rec.read_new_users(str(p))
    assert labels == ["anna b", "zed", "09"] and lists == [[5, 2], [7, 7], [1]]
    for bad in ("a\t1\tx\n", "a 1\n", "a\tone\n", "\t3\n"):
        q = tmp_path / "bad.tsv"
        q.write_text("ok\t1\n" + bad)
        with pytest.raises(ValueError, match="bad.tsv:2"):
            train_rec.read_new_users(str(q))


def test_cli_flag_and_models():
    a = train_rec.parse_args(["--rec", "vbpr"])
    assert a.new_users is None and a.fold_steps == 30 and a.fold_negatives == 4
    for rec in ("bprmf", "vbpr", "grad_fashion"):
        a = train_rec.parse_args(["--rec", rec, "--new_users", "n.tsv", "--fold_steps", "7", "--fold_negatives", "2"])
        assert a.new_users == "n.tsv" and a.fold_steps == 7 and a.fold_negatives == 2
    for argv in (["--rec", "acf", "--new_users", "n.tsv"], ["--rec", "attentive_fashion", "--new_users", "n.tsv"],
                 ["--rec", "vbpr", "--new_users", "n.tsv", "--fold_steps", "0"],
                 ["--rec", "vbpr", "--new_users", "n.tsv", "--fold_negatives", "0"]):
        with pytest.raises(SystemExit):
            train_rec.parse_args(argv)
    with pytest.raises(NotImplementedError):
        train_rec.train(["--rec", "vbpr", "--new_users", "n.tsv", "--world_size", "2"])
