"""Diversified lists without a GPU: tests/diversify_ref.py (the float64 / float32 restatement of bprx_diversify's definition) on a
hand-worked case and on its invariants, the binding and the library's export, the command line, the div-* path names and the
rows ranking.write_diverse writes."""
import io
import os
import re

import numpy as np
import pytest
import torch

import diversify_ref as R
import similar_ref as S
from fashionvisualexpl_recommend_amd import _ffi, ranking, train_rec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- binding and export --------------------------------------------------------------------------------------------------------
def test_the_binding_declares_and_the_library_exports_the_entry():
    header = open(os.path.join(REPO, "include", "bprx.h")).read()
    lib = _ffi.lib()
    assert "bprx_diversify" in _ffi.EXPORTS and re.search(r"BPRX_API int bprx_diversify\(", header)
    fn = lib.bprx_diversify                                   # AttributeError: the library does not export it
    assert len(fn.argtypes) == 14
    assert "#define BPRX_ABI_VERSION 6" in header and _ffi.ABI_VERSION == 6      # purely additive
    assert lib.bprx_diversify(None, 0, None, 0, 1, None, None, 1, 0.5, None, None, None, None, None) == _ffi.E_INVALID


# ---- the reference: a hand-worked case -----------------------------------------------------------------------------------------
def _hand():
    """A = (1, 0), B = (2, 0) (A's direction), C = (0, 1), D = (1, 1); scores 4, 3, 2, 1 -> rel 1, 2/3, 1/3, 0."""
    z = np.array([[1, 0], [2, 0], [0, 1], [1, 1]], np.float64)
    return np.array([10, 11, 12, 13]), np.array([4, 3, 2, 1], np.float32), z


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hand_worked_four_candidates(dtype):
    ids, vals, z = _hand()
    h = np.sqrt(0.5)
    # theta = 0.5.  step 0: obj = rel / 2 -> A.  pen: B 1, C 0, D h.  step 1: B 1/3 - 1/2, C 1/6 - 0, D 0 - h/2 -> C.
    # step 2: pen B max(1, 0) = 1, D max(h, h) = h: B -1/6, D -h/2 -> B (pen 1).  step 3: D (pen h).
    r = R.mmr(ids, vals, z, 4, 0.5, dtype)
    tol = 1e-12 if dtype is np.float64 else 1e-6
    assert r["pos"].tolist() == [0, 2, 1, 3] and r["idx"].tolist() == [10, 12, 11, 13] and r["val"].tolist() == [4, 2, 3, 1]
    assert np.allclose(r["pen"], [0, 0, 1, h], atol=tol)
    assert np.allclose(r["obj"][0], [0.5, 1 / 3, 1 / 6, 0], atol=tol)
    assert np.isnan(r["obj"][1][0]) and np.allclose(r["obj"][1][1:], [1 / 3 - 0.5, 1 / 6, -h / 2], atol=tol)
    assert np.allclose(r["obj"][2][[1, 3]], [-1 / 6, -h / 2], atol=tol) and np.isnan(r["obj"][2][[0, 2]]).all()
    # pairs: AC 0, AB 1, CB 0, DA h, DC h, DB h
    assert abs(float(r["ild"]) - (1 - (1 + 3 * h) / 6)) <= tol
    # K = 2 stops after A, C: orthogonal rows, ild 1; the rest of the slots are empty
    r2 = R.mmr(ids, vals, z, 2, 0.5, dtype)
    assert r2["idx"].tolist() == [10, 12] and abs(float(r2["ild"]) - 1.0) <= tol
    # theta = 1: relevance plays no part; the first pick is the lowest position (all objectives 0), then the least similar
    r3 = R.mmr(ids, vals, z, 3, 1.0, dtype)
    assert r3["pos"].tolist() == [0, 2, 3]
    # a replay of another list: the objectives are conditioned on the given prefix
    f = R.mmr(ids, vals, z, 4, 0.5, dtype, follow=[1, 0])
    assert f["pos"].tolist() == [1, 0] and np.allclose(f["obj"][1][[0, 2, 3]], [0.5 - 0.5, 1 / 6, -h / 2], atol=tol)
    assert abs(float(f["pen"][1]) - 1.0) <= tol and abs(float(f["ild"])) <= tol


# ---- the reference: invariants on random pools ---------------------------------------------------------------------------------
def _random_pool(seed, I=50, N=24, space="both", tail=0):
    rs = np.random.RandomState(seed)
    t = dict(Gi=rs.standard_normal((I, 5)).astype(np.float32), F=rs.standard_normal((I, 9)).astype(np.float32),
             E=rs.standard_normal((9, 4)).astype(np.float32), Bp=rs.standard_normal(9).astype(np.float32))
    t["Gi"][19], t["F"][19] = t["Gi"][7], t["F"][7]            # twins
    z = S.item_vectors(t, space, "fp32", torch.float64)
    ids = rs.permutation(I)[:N].astype(np.int64)
    vals = np.sort(rs.standard_normal(N).astype(np.float32))[::-1].copy()
    if tail:
        ids[N - tail:N - tail // 2] = -1                       # both ways to say "no candidate"
        vals[N - tail // 2:] = -np.inf
    return ids, vals, z


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("space", S.SPACES)
def test_theta_zero_is_the_identity_and_k_equal_n_a_permutation(space, dtype):
    ids, vals, z = _random_pool(1, space=space)
    zp = z[ids]
    for K in (1, 7, 24):
        r = R.mmr(ids, vals, zp, K, 0.0, dtype)
        assert np.array_equal(r["idx"], ids[:K]) and np.array_equal(r["val"].view(np.uint32), vals[:K].view(np.uint32))
    for theta in (0.3, 1.0):
        r = R.mmr(ids, vals, zp, 24, theta, dtype)
        assert sorted(r["idx"].tolist()) == sorted(ids.tolist()) and r["pos"].tolist() != list(range(24))
        assert np.array_equal(r["val"].view(np.uint32), vals[r["pos"]].view(np.uint32))


@pytest.mark.parametrize("theta", [0.5, 0.8, 1.0])
def test_a_twin_of_a_pick_is_redundant_and_demoted(theta):
    ids, vals, z = _random_pool(2)
    ids[0], ids[1] = 7, 19                                     # the two best candidates are twins
    ids[2:] = [i for i in np.random.RandomState(3).permutation(50) if i not in (7, 19)][:22]
    r = R.mmr(ids, vals, z[ids], 24, theta)
    where = r["idx"].tolist().index(19)
    assert r["idx"][0] == 7 and where > 1, "the twin kept the second place"
    assert abs(float(r["pen"][where]) - 1.0) <= 1e-12
    assert R.mmr(ids, vals, z[ids], 24, 0.0)["idx"][1] == 19   # without the penalty it keeps its place


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_slots_without_a_candidate_are_never_returned(dtype):
    ids, vals, z = _random_pool(4, tail=8)
    zp = z[np.maximum(ids, 0)]
    for K, theta in ((24, 0.3), (20, 1.0), (5, 0.0)):
        r = R.mmr(ids, vals, zp, K, theta, dtype)
        T = min(K, 16)
        assert (r["idx"][:T] >= 0).all() and np.isfinite(r["val"][:T]).all() and set(r["pos"].tolist()) <= set(range(16))
        assert (r["idx"][T:] == -1).all() and (r["val"][T:] == 0).all() and (r["pen"][T:] == 0).all() and len(r["pos"]) == T
    flat = R.mmr(ids, np.where(np.isneginf(vals), vals, np.float32(2.5)), zp, 16, 0.0, dtype)      # v_max == v_min: rel = 0
    assert flat["pos"].tolist() == list(range(16))
    none = R.mmr(np.full(4, -1), np.zeros(4, np.float32), np.ones((4, 3)), 3, 0.5, dtype)
    assert (none["idx"] == -1).all() and float(none["ild"]) == 0.0 and len(none["pos"]) == 0


@pytest.mark.parametrize("K", [1, 2, 9, 24])
def test_ild_is_the_direct_pairwise_mean(K):
    ids, vals, z = _random_pool(5)
    r = R.mmr(ids, vals, z[ids], K, 0.4)
    want = R.ild_direct(z[r["idx"][:K]])
    assert abs(float(r["ild"]) - float(want)) <= 1e-13
    assert (K < 2) == (float(r["ild"]) == 0.0)
    r32 = R.mmr(ids, vals, z[ids], K, 0.4, np.float32, follow=r["pos"])
    assert abs(float(r32["ild"]) - float(want)) <= 1e-5 and r32["pen"].dtype == np.float32


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-13), (np.float32, 1e-5)])
def test_the_batched_replay_is_the_list_by_list_one(dtype, tol):
    pools = [(i, v) for i, v, _ in (_random_pool(6 + r, tail=(0, 8, 4)[r]) for r in range(3))]
    z = _random_pool(6)[2]                                     # one catalogue for the three pools
    K = 18
    lists = [R.mmr(i, v, z[np.maximum(i, 0)], K, 0.6) for i, v in pools]
    pos = np.full((3, K), -1, np.int64)
    for r, l in enumerate(lists):
        pos[r, :len(l["pos"])] = l["pos"]
    assert (pos[0] >= 0).all() and (pos[1] >= 0).sum() == 16                         # a full list and a short one
    obj, pen, ild = R.replay(np.stack([i for i, _ in pools]), np.stack([v for _, v in pools]), z, pos, 0.6, dtype)
    for r, l in enumerate(lists):
        T = len(l["pos"])
        one = R.mmr(pools[r][0], pools[r][1], z[np.maximum(pools[r][0], 0)], K, 0.6, dtype, follow=l["pos"])
        assert np.array_equal(np.isnan(obj[r, :T]), np.isnan(one["obj"])) and np.isnan(obj[r, T:]).all()
        assert np.allclose(np.nan_to_num(obj[r, :T]), np.nan_to_num(one["obj"]), rtol=0, atol=tol)
        assert np.allclose(pen[r, :T], one["pen"][:T], rtol=0, atol=tol) and (pen[r, T:] == 0).all()
        assert abs(float(ild[r]) - float(one["ild"])) <= tol


# ---- command line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["--rec", "acf", "--diversify", "0.5"],
    ["--rec", "attentive_fashion", "--diversify", "0.5"],
    ["--rec", "bprmf", "--diversify", "0.5", "--similar_space", "visual"],
    ["--rec", "bprmf", "--diversify", "0.5", "--similar_space", "both"],
    ["--rec", "vbpr", "--dtype", "fp8", "--diversify", "0.5"],
    ["--rec", "vbpr", "--dtype", "fp8", "--diversify", "0.5", "--similar_space", "both"],
    ["--rec", "grad_fashion", "--dtype", "fp8", "--diversify", "0.5", "--similar_space", "visual"],
    ["--rec", "vbpr", "--diversify", "-0.1"],
    ["--rec", "vbpr", "--diversify", "1.5"],
    ["--rec", "vbpr", "--diversify", "nan"],
    ["--rec", "vbpr", "--diversify", "0.5", "--diversify_pool", "19"],
    ["--rec", "vbpr", "--diversify", "0.5", "--diversify_pool", "1025"],
    ["--rec", "vbpr", "--diversify", "0.5", "--top_k", "200"],
], ids=lambda a: " ".join(a))
def test_parse_args_rejects(argv, capsys):
    with pytest.raises(SystemExit):
        train_rec.parse_args(argv)
    err = capsys.readouterr().err
    assert "diversify" in err or "similar_space" in err


def test_parse_args_defaults_and_the_single_gpu_rule():
    for rec, space in (("bprmf", "latent"), ("vbpr", "visual"), ("grad_fashion", "visual")):
        a = train_rec.parse_args(["--rec", rec])
        assert a.diversify == 0.0 and a.diversify_pool == 100
        a = train_rec.parse_args(["--rec", rec, "--diversify", "1"])
        assert a.diversify == 1.0 and a.similar_space == space
    assert train_rec.parse_args(["--rec", "acf"]).diversify == 0.0                              # off: every model trains as before
    assert train_rec.parse_args(["--rec", "vbpr", "--dtype", "fp8", "--diversify_pool", "5"]).diversify_pool == 5     # unread while off
    a = train_rec.parse_args(["--rec", "vbpr", "--dtype", "fp8", "--diversify", "0.25", "--similar_space", "latent", "--top_k", "64",
                              "--diversify_pool", "64"])
    assert (a.diversify, a.diversify_pool, a.similar_space) == (0.25, 64, "latent")
    assert train_rec.parse_args(["--rec", "vbpr", "--diversify", "0.5", "--diversify_pool", "1024"]).diversify_pool == 1024
    with pytest.raises(NotImplementedError, match="diversify"):
        train_rec.train(["--rec", "vbpr", "--diversify", "0.5", "--world_size", "2"])


# ---- models without an item space ---------------------------------------------------------------------------------------------
def test_models_without_an_item_space_refuse():
    from fashionvisualexpl_recommend_amd import models
    for cls in (models.ACF, models.AttentiveFashion):
        obj = cls.__new__(cls)                                         # (no engine is needed to refuse)
        with pytest.raises(NotImplementedError):
            obj.recommend_diverse()
        with pytest.raises(NotImplementedError):
            obj.recommend_new_users([[1, 2]], diversify=0.5)


# ---- files ---------------------------------------------------------------------------------------------------------------------
def test_div_path_names():
    d = os.path.join("res", "rec_results", "toy", "vbpr")
    tail = "batch_64-K_8-lr_0.001-reg_0.0.tsv"
    for f, recs, ild in (("recs-3-" + tail, "div-recs-3-" + tail, "div-ild-3-" + tail),
                         ("best-recs-2-" + tail, "best-div-recs-2-" + tail, "best-div-ild-2-" + tail),
                         ("new-user-recs-3-" + tail, "div-new-user-recs-3-" + tail, "div-new-user-ild-3-" + tail),
                         ("best-new-user-recs-2-" + tail, "best-div-new-user-recs-2-" + tail, "best-div-new-user-ild-2-" + tail)):
        assert ranking.div_paths(os.path.join(d, f)) == (os.path.join(d, recs), os.path.join(d, ild)), f
    assert ranking.div_paths("recs-1-x.tsv") == ("div-recs-1-x.tsv", "div-ild-1-x.tsv")
    with pytest.raises(ValueError):
        ranking.div_paths(os.path.join(d, "sim-3-" + tail))


def test_write_diverse_rows():
    ids = np.array([[4, 9, 2], [7, -1, -1], [-1, -1, -1]], np.int64)
    vals = np.array([[1.5, -0.0, 0.25], [3.0, 0, 0], [0, 0, 0]], np.float32)
    pen = np.array([[0, 0.1, 0.75], [0, 0, 0], [0, 0, 0]], np.float32)
    ild = np.array([0.6, 0, 0], np.float32)
    out, oi = io.StringIO(), io.StringIO()
    ranking.write_diverse(out, oi, ["u a", 8, 9], ids, vals, pen, ild)
    assert out.getvalue() == "u a\t4\t1.5\t0.0\nu a\t9\t-0.0\t0.1\nu a\t2\t0.25\t0.75\n8\t7\t3.0\t0.0\n"
    assert oi.getvalue() == "u a\t0.6\n8\t0.0\n9\t0.0\n"
    # the first three columns of a row are the row write_ranked writes for the same pick
    plain = io.StringIO()
    ranking.write_ranked(plain, ["u a"], ids[:1], vals[:1])
    assert [l.rsplit("\t", 1)[0] for l in out.getvalue().splitlines()[:3]] == plain.getvalue().splitlines()


def test_diversify_rows_uploads_once_and_cuts_k_to_the_pool():
    calls = []

    def entry(pool_idx, pool_val, k):
        calls.append((pool_idx.dtype, pool_val.dtype, tuple(pool_idx.shape), k, pool_idx.is_contiguous()))
        n = pool_idx.shape[0]
        return pool_idx[:, :k].clone(), pool_val[:, :k].clone(), torch.zeros(n, k), torch.ones(n)

    ids = np.arange(12, dtype=np.int64).reshape(2, 6)[:, ::-1]             # (a view: not contiguous)
    vals = np.linspace(1, 0, 12, dtype=np.float32).reshape(2, 6)
    got = ranking.diversify_rows(entry, ids, vals, 4, "cpu")
    assert calls == [(torch.int32, torch.float32, (2, 6), 4, True)]
    assert got[0].dtype == np.int64 and np.array_equal(got[0], ids[:, :4]) and np.array_equal(got[1], vals[:, :4])
    assert got[2].shape == (2, 4) and got[3].tolist() == [1, 1]
    assert ranking.diversify_rows(entry, ids, vals, 9, "cpu")[0].shape == (2, 6) and calls[-1][3] == 6
    empty = ranking.diversify_rows(entry, np.zeros((0, 6), np.int64), np.zeros((0, 6), np.float32), 4, "cpu")
    assert [e.shape for e in empty] == [(0, 4), (0, 4), (0, 4), (0,)] and len(calls) == 2
