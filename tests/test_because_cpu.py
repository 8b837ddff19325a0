"""'Because you own X' without a GPU: tests/because_ref.py (the float64 / float32 restatement of bprx_because's definition) on
hand-made cases, the binding and the library's export, the command line, the because-* path names, the rows
ranking.write_because writes and the grouping of pairs into lists (ranking.because_rows with a stubbed entry)."""
import io
import os
import re

import numpy as np
import pytest
import torch

import because_ref as R
from fashionvisualexpl_recommend_amd import _ffi, ranking, train_rec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- binding and export --------------------------------------------------------------------------------------------------------
def test_the_binding_declares_and_the_library_exports_the_entry():
    header = open(os.path.join(REPO, "include", "bprx.h")).read()
    lib = _ffi.lib()
    assert "bprx_because" in _ffi.EXPORTS and re.search(r"BPRX_API int bprx_because\(", header)
    fn = lib.bprx_because                                     # AttributeError: the library does not export it
    assert len(fn.argtypes) == 16
    assert "#define BPRX_ABI_VERSION 6" in header and _ffi.ABI_VERSION == 6      # purely additive
    assert lib.bprx_because(None, 0, None, 0, None, None, 0, 1, None, None, None, 1, None, None, None, None) == _ffi.E_INVALID


# ---- the reference: hand-made cases --------------------------------------------------------------------------------------------
def _hand():
    """Catalogue: 0 = (1, 0), 1 = (2, 0) (0's direction), 2 = (0, 1), 3 = (1, 1), 4 = (0, 0), 5 = (-1, 0), 6 = (3, 0)."""
    return np.array([[1, 0], [2, 0], [0, 1], [1, 1], [0, 0], [-1, 0], [3, 0]], np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hand_made_order_ties_self_and_short_histories(dtype):
    z = _hand()
    h = np.sqrt(0.5)
    tol = 1e-12 if dtype is np.float64 else 1e-6
    # item 0 against the history (3, 6, 2, 1, 5): cosines h, 1, 0, 1, -1.  6 and 1 tie at 1: the lower position (6) first
    r = R.because([0], [3, 6, 2, 1, 5], z, 3, dtype)
    assert r["pos"].tolist() == [[1, 3, 0]] and r["item"].tolist() == [[6, 1, 3]] and r["cnt"].tolist() == [5]
    assert np.allclose(r["cos"], [[1, 1, h]], atol=tol) and r["cos"].dtype == dtype
    assert r["cos"][0, 0] == r["cos"][0, 1]                                          # (a true tie, not a near one)
    assert np.allclose(r["all"], [[h, 1, 0, 1, -1]], atol=tol)
    # the same history the other way round: now item 1 (position 1) leads the tie
    assert R.because([0], [5, 1, 2, 6, 3], z, 2, dtype)["item"].tolist() == [[1, 6]]
    # the explained item inside its own history is skipped, wherever and however often it stands
    r = R.because([6, 2], [6, 1, 6, 2], z, 4, dtype)
    assert r["item"].tolist() == [[1, 2, -1, -1], [6, 1, 6, -1]] and r["cnt"].tolist() == [2, 3]
    assert r["pos"].tolist() == [[1, 3, -1, -1], [0, 1, 2, -1]]                       # equal ids are two entries: by position
    assert np.isnan(r["all"][0, [0, 2]]).all() and np.isnan(r["all"][1, 3])
    # a row from outside the catalogue is nobody's own item: nothing is skipped
    r = R.because([0], [0, 1, 0, 2], z, 4, dtype, zq=np.array([[1.0, 0.0]]))
    assert r["item"].tolist() == [[0, 1, 0, 2]] and r["cnt"].tolist() == [4]
    # empty history, L > M, an empty slot, a zero row (cosine 0 with everything, never nan)
    r = R.because([0, 3], [], z, 2, dtype)
    assert (r["item"] == -1).all() and (r["cos"] == 0).all() and r["cnt"].tolist() == [0, 0] and r["all"].shape == (2, 0)
    r = R.because([3, -1, 4], [0, 2], z, 5, dtype)
    assert r["item"].tolist() == [[0, 2, -1, -1, -1], [-1] * 5, [0, 2, -1, -1, -1]] and r["cnt"].tolist() == [2, 0, 2]
    assert np.allclose(r["cos"][0, :2], [h, h], atol=tol) and (r["cos"][0, 2:] == 0).all() and (r["cos"][1:] == 0).all()
    # a history that is only the item itself: no candidate
    assert R.because([2], [2, 2], z, 3, dtype)["cnt"].tolist() == [0]


def test_minus_zero_ties_with_plus_zero():
    cos = np.array([0.0, -0.0, 0.5, -0.0, 0.0], np.float32)
    assert R.nearest(cos, np.ones(5, bool), 5).tolist() == [2, 0, 1, 3, 4]
    assert R.nearest(cos, np.array([0, 1, 0, 1, 1], bool), 2).tolist() == [1, 3]


def test_the_batched_form_is_the_list_by_list_one():
    rs = np.random.RandomState(3)
    z = rs.standard_normal((40, 6))
    lists = rs.randint(-1, 40, (5, 7))
    hists = [rs.permutation(40)[:h] for h in (0, 1, 9, 30, 2)]
    item, cos, cnt, pos, allc = R.because_lists(lists, hists, z, 4)
    assert allc.shape == (5, 7, 30)
    for r in range(5):
        one = R.because(lists[r], hists[r], z, 4)
        assert np.array_equal(item[r], one["item"]) and np.array_equal(cos[r], one["cos"]) and np.array_equal(cnt[r], one["cnt"])
        assert np.array_equal(pos[r], one["pos"]) and np.isnan(allc[r, :, len(hists[r]):]).all()


# ---- command line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["--rec", "acf", "--because", "3"],
    ["--rec", "attentive_fashion", "--because", "3"],
    ["--rec", "bprmf", "--because", "3", "--similar_space", "visual"],
    ["--rec", "bprmf", "--because", "3", "--similar_space", "both"],
    ["--rec", "vbpr", "--dtype", "fp8", "--because", "3"],
    ["--rec", "vbpr", "--dtype", "fp8", "--because", "3", "--similar_space", "both"],
    ["--rec", "grad_fashion", "--dtype", "fp8", "--because", "3", "--similar_space", "visual"],
    ["--rec", "vbpr", "--because", "-1"],
    ["--rec", "vbpr", "--because", "33"],
], ids=lambda a: " ".join(a))
def test_parse_args_rejects(argv, capsys):
    with pytest.raises(SystemExit):
        train_rec.parse_args(argv)
    err = capsys.readouterr().err
    assert "because" in err or "similar_space" in err


def test_parse_args_defaults_and_the_single_gpu_rule():
    for rec, space in (("bprmf", "latent"), ("vbpr", "visual"), ("grad_fashion", "visual")):
        assert train_rec.parse_args(["--rec", rec]).because == 0
        a = train_rec.parse_args(["--rec", rec, "--because", "32"])
        assert a.because == 32 and a.similar_space == space
    assert train_rec.parse_args(["--rec", "acf"]).because == 0                                 # off: every model trains as before
    a = train_rec.parse_args(["--rec", "vbpr", "--dtype", "fp8", "--because", "1", "--similar_space", "latent"])
    assert (a.because, a.similar_space) == (1, "latent")
    a = train_rec.parse_args(["--rec", "vbpr", "--because", "5", "--similar_space", "both", "--feat_explain", "4", "--diversify", "0.5"])
    assert (a.because, a.similar_space, a.feat_explain, a.diversify) == (5, "both", 4, 0.5)    # combines freely
    with pytest.raises(NotImplementedError, match="because"):
        train_rec.train(["--rec", "vbpr", "--because", "3", "--world_size", "2"])
    with pytest.raises(ValueError, match="because"):
        train_rec.train(["--rec", "vbpr", "--because", "3", "--top_k", "1025"])


# ---- models without an item space ---------------------------------------------------------------------------------------------
def test_models_without_an_item_space_name_their_own_flag():
    from fashionvisualexpl_recommend_amd import models
    for cls, flag in ((models.ACF, "--acf_explain"), (models.AttentiveFashion, "--af_explain")):
        obj = cls.__new__(cls)                                         # (no engine is needed to refuse)
        with pytest.raises(NotImplementedError, match=flag):
            obj.because([0], [1])


# ---- files ---------------------------------------------------------------------------------------------------------------------
def test_because_path_names():
    d = os.path.join("res", "rec_results", "toy", "vbpr")
    tail = "batch_64-K_8-lr_0.001-reg_0.0.tsv"
    for f, want in (("recs-3-" + tail, "because-3-" + tail),
                    ("best-recs-2-" + tail, "best-because-2-" + tail),
                    ("new-user-recs-3-" + tail, "because-new-user-recs-3-" + tail),
                    ("best-new-user-recs-2-" + tail, "best-because-new-user-recs-2-" + tail),
                    ("new-recs-3-" + tail, "because-new-recs-3-" + tail),
                    ("best-new-recs-2-" + tail, "best-because-new-recs-2-" + tail)):
        assert ranking.because_paths(os.path.join(d, f)) == os.path.join(d, want), f
    assert ranking.because_paths("recs-1-x.tsv") == "because-1-x.tsv"
    for bad in ("sim-3-" + tail, "div-recs-3-" + tail, "expl-3-" + tail):
        with pytest.raises(ValueError):
            ranking.because_paths(os.path.join(d, bad))


def test_write_because_rows():
    ids = np.array([[4, 9], [7, 3]], np.int64)
    vals = np.array([[1.5, -0.0], [3.0, 0.25]], np.float32)
    hist = np.array([[[8, 2, -1], [-1, -1, -1]], [[5, 6, 1], [2, -1, -1]]], np.int64)
    cos = np.array([[[0.75, -0.0, 0], [0, 0, 0]], [[1.0, 0.5, -0.25], [1e-8, 0, 0]]], np.float32)
    out = io.StringIO()
    ranking.write_because(out, ["u a", 8], ids, vals, hist, cos)
    assert out.getvalue() == ("u a\t4\t1.5\t0\t8\t0.75\nu a\t4\t1.5\t1\t2\t-0.0\n"
                              "u a\t9\t-0.0\t-1\t-1\t0.0\n"                                    # no candidate: the pair is still named
                              "8\t7\t3.0\t0\t5\t1.0\n8\t7\t3.0\t1\t6\t0.5\n8\t7\t3.0\t2\t1\t-0.25\n"
                              "8\t3\t0.25\t0\t2\t1e-08\n")
    # the first three columns of a pair's rows are the row write_ranked writes for it, pair by pair in its order
    plain = io.StringIO()
    ranking.write_ranked(plain, ["u a", 8], ids, vals)
    heads = [l.rsplit("\t", 3)[0] for l in out.getvalue().splitlines()]
    assert list(dict.fromkeys(heads)) == plain.getvalue().splitlines()
    empty = io.StringIO()
    ranking.write_because(empty, [1], ids[:1], vals[:1], np.zeros((1, 2, 0), np.int64), np.zeros((1, 2, 0), np.float32))
    assert empty.getvalue() == "1\t4\t1.5\t-1\t-1\t0.0\n1\t9\t-0.0\t-1\t-1\t0.0\n"


# ---- pairs -> lists ------------------------------------------------------------------------------------------------------------
def _stub(calls, L):
    """An entry that answers slot (r, q) with item = 1000 r + q, cos = the slot's list entry, cnt = the history's length, and
    records what it was given."""
    def entry(list_idx, csr):
        ptr, items = csr
        assert list_idx.dtype == torch.int32 and list_idx.is_contiguous() and ptr.dtype == torch.int64 and items.dtype == torch.int32
        n, K = list_idx.shape
        calls.append((list_idx.numpy().copy(), ptr.numpy().copy(), items.numpy().copy()))
        item = (1000 * torch.arange(n)[:, None, None] + torch.arange(K)[None, :, None] + torch.zeros(1, 1, L)).to(torch.int32)
        cos = list_idx[:, :, None].float() + torch.zeros(1, 1, L)
        cnt = (ptr[1:] - ptr[:-1])[:, None].expand(n, K).to(torch.int32)
        return item, cos, cnt
    return entry


def test_pairs_become_lists_by_runs_of_equal_users():
    lists = [[5, 6, 5], [], [7], [1, 2, 3, 3]]
    users = [3, 3, 0, 0, 0, 3, 2]
    items = [10, 11, 12, 13, 14, 15, 16]
    for dedup, hist3, hist0 in ((False, [1, 2, 3, 3], [5, 6, 5]), (True, [1, 2, 3], [5, 6])):
        calls = []
        hist, cos, cnt = ranking.because_rows(_stub(calls, 2), users, items, lists, 2, "cpu", dedup)
        assert len(calls) == 1
        li, ptr, its = calls[0]
        assert li.tolist() == [[10, 11, -1], [12, 13, 14], [15, -1, -1], [16, -1, -1]]          # runs, padded with -1
        want = [hist3, hist0, hist3, [7]]                                                       # a user's second run: the list again
        assert ptr.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist() and its.tolist() == [i for w in want for i in w]
        assert hist.dtype == np.int64 and hist.shape == (7, 2) and cos.shape == (7, 2) and cnt.shape == (7,)
        assert hist[:, 0].tolist() == [0, 1, 1000, 1001, 1002, 2000, 3000]                      # each pair reads its own slot
        assert cos[:, 1].tolist() == [float(i) for i in items]
        assert cnt.tolist() == [len(hist3)] * 2 + [len(hist0)] * 3 + [len(hist3), 1]


def test_a_run_is_split_at_1024_entries():
    calls = []
    users = [4] * 2050 + [1] * 3
    items = list(range(2050)) + [7, 8, 9]
    lists = {4: [2, 3], 1: [5]}
    hist, cos, cnt = ranking.because_rows(_stub(calls, 1), users, items, lists, 1, "cpu")
    li, ptr, its = calls[0]
    assert li.shape == (4, 1024) and ptr.tolist() == [0, 2, 4, 6, 7] and its.tolist() == [2, 3, 2, 3, 2, 3, 5]
    assert li[0].tolist() == list(range(1024)) and li[1].tolist() == list(range(1024, 2048))
    assert li[2, :2].tolist() == [2048, 2049] and (li[2, 2:] == -1).all() and li[3, :3].tolist() == [7, 8, 9] and (li[3, 3:] == -1).all()
    assert cos[:, 0].tolist() == [float(i) for i in items]
    assert hist[[0, 1023, 1024, 2047, 2048, 2050], 0].tolist() == [0, 1023, 1000, 2023, 2000, 3000]
    assert cnt.tolist() == [2] * 2050 + [1] * 3
    # exactly 1024: one list; no pairs: the entry is not called
    calls.clear()
    ranking.because_rows(_stub(calls, 1), [0] * 1024, list(range(1024)), [[1]], 1, "cpu")
    assert calls[0][0].shape == (1, 1024)
    calls.clear()
    hist, cos, cnt = ranking.because_rows(_stub(calls, 3), [], [], [[1]], 3, "cpu")
    assert not calls and hist.shape == (0, 3) and cos.shape == (0, 3) and cnt.shape == (0,)
    with pytest.raises(ValueError):
        ranking.because_rows(_stub(calls, 3), [0, 0], [1], [[1]], 3, "cpu")
