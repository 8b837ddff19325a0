"""Warm items without a GPU: the pair sampler, the restatement (tests/item_fold_ref.py) against central differences of its own loss
and against the oracle's train step, the inputs of tests/test_gpu_item_fold.py (so that the GPU test cannot hide behind them), the
three new symbols (declared, bound, exported, ABI still 6; a NULL handle is rejected), the names of the warm-* files and the rules
of --warm_items."""
import os
import re

import numpy as np
import pytest

import item_fold_cases as C
import item_fold_ref as R
from fashionvisualexpl_recommend_amd import _ffi, ranking, train_rec
from fashionvisualexpl_recommend_amd.models import draw_item_fold_pairs
from oracle import oracle as orc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bprx.h")
SYMBOLS = {"bprx_fold_in_items": 15, "bprx_score_warm_block": 9, "bprx_audience_warm_block": 9}
STEP_TOL = {"sgd": dict(rtol=2e-6, atol=2e-7), "adam_tf23": dict(rtol=2e-4, atol=2e-6)}      # tests/test_oracle_step.py's


# ---- the pair sampler --------------------------------------------------------------------------------------------------------
def test_draw_item_fold_pairs():
    I = 30
    train = [[3, 4, 5], [], list(range(I)), [7], [9, 9, 2], [1, 2], [0]]
    buyers = [[0, 4, 0], [], [2], [1, 3]]
    ptr, user, other, role = draw_item_fold_pairs(buyers, train, I, 4, seed=1)
    assert ptr.dtype == np.int64 and user.dtype == other.dtype == role.dtype == np.int32
    # item 0: two distinct buyers; item 1: none; item 2: its buyer's list covers the catalogue; item 3: a buyer with an empty list
    assert ptr.tolist() == [0, 16, 16, 16, 32]
    for r, who in enumerate(buyers):
        u, o, ro = (x[ptr[r]:ptr[r + 1]] for x in (user, other, role))
        n0 = int((ro == 0).sum())
        assert n0 == len(u) - n0                                              # roles balanced
        assert ro[:n0].tolist() == [0] * n0                                   # role 0 first
        assert u[:n0].tolist() == np.repeat(list(dict.fromkeys(who)), 4)[:n0].tolist()     # buyers in first-appearance order
        for uu, oo in zip(u[:n0], o[:n0]):
            assert oo not in train[uu] and 0 <= oo < I                        # role-0 negatives outside the buyer's list
        for uu, oo in zip(u[n0:], o[n0:]):
            assert uu not in who and train[uu] and oo in train[uu]            # role-1 users: no buyers, o' from their own list
    again = draw_item_fold_pairs(buyers, train, I, 4, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip((ptr, user, other, role), again))
    assert not np.array_equal(draw_item_fold_pairs(buyers, train, I, 4, seed=2)[2], other)
    # every other user is a buyer or has no list: no role-1 pairs
    p2, u2, _, r2 = draw_item_fold_pairs([[0, 2, 3, 4, 5, 6]], train, I, 2, seed=0)
    assert p2.tolist() == [0, 10] and not r2.any() and 2 not in u2
    e = draw_item_fold_pairs([], train, I, 4, seed=0)
    assert e[0].tolist() == [0] and all(x.size == 0 for x in e[1:])
    for bad_buyers, bad_train in (([[7]], train), ([[-1]], train), ([[0]], [[I]]), ([[0]], [[-1]])):
        with pytest.raises(ValueError):
            draw_item_fold_pairs(bad_buyers, bad_train, I, 4, seed=0)
    with pytest.raises(ValueError):
        draw_item_fold_pairs(buyers, train, I, 0, seed=0)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", [(5, 0), (7, 6)])
def test_gradient_of_the_restatement_is_the_derivative_of_its_loss(k, d):
    t = C.tables(k, d, seed=11)
    P, Pn = C.host_projections(t)
    rs = np.random.RandomState(12)
    n = 23
    user, other, role = rs.randint(C.U, size=n), rs.randint(C.I, size=n), rs.randint(2, size=n)
    c64 = lambda x: None if x is None else np.asarray(x, np.float64)
    D, dc = R.pair_terms(c64(t["Gu"]), c64(t.get("Tu")), c64(t["Gi"]), c64(t["Bi"]), c64(P), None if Pn is None else c64(Pn[3]),
                         user, other, role)
    npos = int((role == 0).sum())
    rv = np.full(k + 1, float(n))
    rv[k] = npos + 0.1 * (n - npos)
    w = rs.standard_normal(k + 1) * 0.3
    _, g = R.loss_and_grad(w, D, dc, rv, 1e-2)
    h = 1e-6
    fd = np.array([(R.loss_and_grad(w + h * e, D, dc, rv, 1e-2)[0] - R.loss_and_grad(w - h * e, D, dc, rv, 1e-2)[0]) / (2 * h)
                   for e in np.eye(k + 1)])
    assert np.abs(fd - g).max() <= 1e-8 * max(1.0, np.abs(g).max())
    assert 0 < npos < n and np.abs(g).min() > 0


@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
@pytest.mark.parametrize("model", ["bprmf", "vbpr"])
def test_one_step_of_the_restatement_is_the_oracles_step_for_that_item(model, opt):
    """T = 1 from a catalogue item's own rows, the batch having that item once per triplet in either role: the restatement moves
    [Gi | Bi] as oracle.OracleModel.step moves them (adam_tf23 from zero slots)."""
    k, d = (8, 6) if model == "vbpr" else (8, 0)
    t = C.tables(k, d, seed=21, users=12)
    P, _ = C.host_projections(t)
    rs = np.random.RandomState(22)
    it, B, lr, reg = 17, 23, 0.05, 1e-2
    user, role = rs.randint(12, size=B), rs.randint(2, size=B)
    other = rs.choice(np.delete(np.arange(C.I), it), size=B)
    pos, neg = np.where(role == 0, it, other), np.where(role == 0, other, it)
    m = orc.OracleModel(**C.bound(t))
    m.step(user, pos, neg, opt, lr, reg)
    r = R.fold_in_items(t["Gu"], t.get("Tu"), t["Gi"], t["Bi"], P, None if P is None else P[it:it + 1], [0, B], user, other, role,
                        t["Gi"][it:it + 1], t["Bi"][it:it + 1], 1, lr, reg, opt)
    np.testing.assert_allclose(m.Gi[it], r["Gi"][0], err_msg="Gi", **STEP_TOL[opt])
    np.testing.assert_allclose(m.Bi[it], r["Bi"][0], err_msg="Bi", **STEP_TOL[opt])
    assert np.abs(m.Gi[it] - t["Gi"][it]).max() > 1e-4 and abs(m.Bi[it] - t["Bi"][it]) > 1e-4


def test_an_item_without_pairs_keeps_its_rows():
    t = C.tables(5, 0, seed=5)
    rs = np.random.RandomState(6)
    W0 = (rs.standard_normal((3, 6)) * 0.3).astype(np.float32)
    a = ([0, 7, 7, 12], rs.randint(C.U, size=12), rs.randint(C.I, size=12), rs.randint(2, size=12), W0)
    for hp in (C.SGD, C.ADAM):
        r64, r32 = (C.restate(t, None, None, *a, hp, dt) for dt in (np.float64, np.float32))
        assert r64["Gi"].dtype == np.float64 and r32["Bi"].dtype == np.float32
        assert np.array_equal(C.rows(r32)[1], W0[1]) and r64["loss"][1] == 0 and r64["grads"][1].shape == (0, 6)
        assert r64["grads"][0].shape == (hp["steps"], 6) and (r64["loss"][[0, 2]] > 0).all()
        assert 0 < np.abs(C.rows(r64) - C.rows(r32)).max() < 1e-5


# ---- the inputs of the GPU test ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", C.WIDTHS)
def test_inputs_of_the_gpu_test(k, d):
    """What tests/test_gpu_item_fold.py relies on, with the projections made on the host: every item's float64 sgd loss falls,
    Adam's left-out share is at most 2 %, and the float32 restatement stays within 5e-6 of the float64 one on the kept Adam
    entries (no kept entry sits at the threshold)."""
    seed = C.SEEDS[(k, d)]
    t = C.tables(k, d, seed)
    P, Pn = C.host_projections(t)
    a = C.items(t, P, Pn, k, d, seed)
    ptr, user, other, role, W0 = a
    cnt = np.diff(ptr)
    assert len(cnt) == C.N_NEW and cnt[:10].tolist() == [0, 1, 3, 4, 5, 17, 64, 65, 200, 3000] and cnt[10:].min() >= 1 and cnt[10:].max() <= 40
    assert 0 < role.mean() < 1 and user.max() < C.U and other.max() < C.I
    q = int(ptr[7])
    assert (user[q + 2], other[q + 2], role[q + 2]) == (user[q + 3], other[q + 3], role[q + 3])
    q = int(ptr[6])
    assert (user[q + 4], other[q + 4]) == (user[q + 5], other[q + 5]) and role[q + 4] != role[q + 5]
    has = cnt > 0
    s64, s32 = (C.restate(t, P, Pn, *a, C.SGD, dt) for dt in (np.float64, np.float32))
    assert (s64["loss"][has] < s64["loss_first"][has]).all()
    sdev = np.abs(C.rows(s64) - C.rows(s32)).max()
    a64, a32 = (C.restate(t, P, Pn, *a, C.ADAM, dt) for dt in (np.float64, np.float32))
    assert (a64["loss"][has] < a64["loss_first"][has]).all()
    keep, share = C.adam_keep(a64, ptr)
    adev = np.abs(C.rows(a64)[keep] - C.rows(a32)[keep]).max()
    print("k=%d d=%d seed=%d: sgd float32 deviation %.3e, adam left-out share %.4f, adam float32 deviation (kept) %.3e" % (
        k, d, seed, sdev, share, adev))
    assert share <= 0.02
    assert adev <= 5e-6
    assert sdev <= 5e-6


# ---- binding, names, CLI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    hdr = open(HEADER).read()
    assert re.search(r"#define\s+BPRX_ABI_VERSION\s+6\b", hdr) and _ffi.ABI_VERSION == 6
    lib = _ffi.lib()
    for name, nargs in SYMBOLS.items():
        assert re.search(r"BPRX_API\s+int\s+%s\s*\(" % name, hdr), name
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs, name


def test_a_null_handle_is_rejected():
    lib = _ffi.lib()
    assert lib.bprx_fold_in_items(None, None, None, None, None, 0, None, 1, 0.1, 0.0, 0, None, None, None, None) == _ffi.E_INVALID
    assert lib.bprx_score_warm_block(None, 0, 0, None, None, None, 0, None, None) == _ffi.E_INVALID
    assert lib.bprx_audience_warm_block(None, None, None, None, 0, 0, 0, None, None) == _ffi.E_INVALID


def test_warm_file_names():
    assert list(ranking.WARM_FILES) == ["warm-recs", "warm-audience"]
    assert not set(ranking.WARM_FILES) & (set(ranking.RUN_FILES) | set(ranking.ITEM_FILES))
    assert ranking.warm_file("r/recs-3-b_1-K_8.tsv", "warm-recs") == "r/warm-recs-3-b_1-K_8.tsv"
    assert ranking.warm_file("r/best-recs-3-b_1-K_8.tsv", "warm-audience") == "r/best-warm-audience-3-b_1-K_8.tsv"
    assert ranking.warm_file("recs-1-x.tsv", "warm-recs") == "warm-recs-1-x.tsv"
    for path, kind in (("r/recs-3-x.tsv", "recs"), ("r/recs-3-x.tsv", "audience"), ("r/new-recs-3-x.tsv", "warm-recs"),
                       ("r/warm-recs-3-x.tsv", "warm-recs"), ("r/other.tsv", "warm-recs")):
        with pytest.raises(ValueError):
            ranking.warm_file(path, kind)


def test_warm_items_file(tmp_path):
    p = tmp_path / "warm.tsv"
    p.write_text("2\t5\n0\t7\n\n2\t9\n2\t5\n")
    assert train_rec.read_warm_items(str(p)) == [[7], [], [5, 9, 5]]
    assert train_rec.read_warm_items(str(p), 5) == [[7], [], [5, 9, 5], [], []]
    with pytest.raises(ValueError, match="warm.tsv:1: row 2 is past"):
        train_rec.read_warm_items(str(p), 2)
    for bad in ("1\t2\t3\n", "1 2\n", "a\t1\n", "1\tb\n", "-1\t3\n", "1\t-3\n", "\t3\n"):
        q = tmp_path / "bad.tsv"
        q.write_text("0\t1\n" + bad)
        with pytest.raises(ValueError, match="bad.tsv:2"):
            train_rec.read_warm_items(str(q))
    (tmp_path / "empty.tsv").write_text("\n")
    assert train_rec.read_warm_items(str(tmp_path / "empty.tsv")) == [] and train_rec.read_warm_items(str(tmp_path / "empty.tsv"), 2) == [[], []]


def test_cli_flag_and_models(tmp_path):
    w = tmp_path / "warm.tsv"
    w.write_text("0\t1\n")
    assert train_rec.parse_args(["--rec", "vbpr"]).warm_items is None
    a = train_rec.parse_args(["--rec", "bprmf", "--warm_items", str(w), "--fold_steps", "7", "--fold_negatives", "2"])
    assert a.warm_items == str(w) and a.fold_steps == 7 and a.fold_negatives == 2
    assert train_rec.parse_args(["--rec", "vbpr", "--warm_items", str(w), "--new_items", "f.npy"]).new_items == ["f.npy"]
    assert train_rec.parse_args(["--rec", "grad_fashion", "--warm_items", str(w), "--new_items", "c.npy", "e.npy"]).warm_items == str(w)
    bad = tmp_path / "bad.tsv"
    bad.write_text("zero\t1\n")
    for argv in (["--rec", "acf", "--warm_items", str(w)], ["--rec", "attentive_fashion", "--warm_items", str(w)],
                 ["--rec", "vbpr", "--warm_items", str(w)], ["--rec", "grad_fashion", "--warm_items", str(w)],
                 ["--rec", "bprmf", "--warm_items", str(bad)], ["--rec", "bprmf", "--warm_items", str(tmp_path / "missing.tsv")],
                 ["--rec", "bprmf", "--warm_items", str(w), "--fold_steps", "0"]):
        with pytest.raises(SystemExit):
            train_rec.parse_args(argv)
    with pytest.raises(NotImplementedError):
        train_rec.train(["--rec", "bprmf", "--warm_items", str(w), "--world_size", "2"])
    np.save(str(tmp_path / "new.npy"), np.zeros((2, 4), np.float32))
    (tmp_path / "past.tsv").write_text("1\t0\n2\t0\n")
    with pytest.raises(ValueError, match="past.tsv:2: row 2 is past the table of 2"):       # before anything is loaded or trained
        train_rec.train(["--rec", "vbpr", "--warm_items", str(tmp_path / "past.tsv"), "--new_items", str(tmp_path / "new.npy")])
