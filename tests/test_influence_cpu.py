"""Influence explanations without a GPU: the binding and the library's export, identities of tests/influence_ref.py (the float64 /
float32 restatement of bprx_influence's definition), the claim itself -- influence against an actual leave-one-entry-out refit, on
the restatement alone -- the influence-* path names, the command line, the rows ranking.write_influence writes and the grouping
of pairs into lists (ranking.influence_rows with a stubbed entry)."""
import io
import os
import re

import numpy as np
import pytest
import torch

import influence_ref as R
from fashionvisualexpl_recommend_amd import _ffi, ranking, train_rec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- binding and export --------------------------------------------------------------------------------------------------------
def test_the_binding_declares_and_the_library_exports_the_entry():
    header = open(os.path.join(REPO, "include", "bprx.h")).read()
    lib = _ffi.lib()
    assert "bprx_influence" in _ffi.EXPORTS and re.search(r"BPRX_API int bprx_influence\(", header)
    fn = lib.bprx_influence                                   # AttributeError: the library does not export it
    assert len(fn.argtypes) == 21
    assert "#define BPRX_ABI_VERSION 6" in header and _ffi.ABI_VERSION == 6      # purely additive
    assert "#define BPRX_INFLUENCE_MAX_WIDTH 160" in header
    assert lib.bprx_influence(None, None, None, 0, None, None, None, 1, 0.0, 1.0, 1, None, 1, None, None, None, None, None, 1, None,
                              None) == _ffi.E_INVALID
    from fashionvisualexpl_recommend_amd import build
    assert "bprx_influence.hip" in build.SOURCES


# ---- the reference -------------------------------------------------------------------------------------------------------------
def _case(seed, n, k, d, counts, pe, I=50, short=0):
    rs = np.random.RandomState(seed)
    g = lambda *s: (rs.standard_normal(s) * 0.4).astype(np.float32)
    Gi, Bi, P = g(I, k), g(I), (g(I, d + 1) if d else None)
    Gu, Tu = g(n, k), (g(n, d) if d else None)
    ptr, pos, neg = [0], [], []
    for E in counts:
        h = rs.randint(I, size=E)
        m = max(E * pe - short, 0) if E else 0
        pos.append(np.repeat(h, pe)[:m]); neg.append(rs.randint(I, size=m)); ptr.append(ptr[-1] + m)
    return Gi, Bi, P, Gu, Tu, np.asarray(ptr, np.int64), np.concatenate(pos), np.concatenate(neg)


def test_a_short_last_group_is_an_entry_and_a_row_without_pairs_gives_nothing():
    Gi, Bi, P, Gu, Tu, ptr, pos, neg = _case(1, 3, 4, 3, [3, 0, 1], 4, short=3)
    assert np.diff(ptr).tolist() == [9, 0, 1]
    lists = np.array([[1, -1, 7], [2, 3, 4], [5, 6, -1]])
    r = R.influence(Gi, Bi, P, Gu, Tu, ptr, pos, neg, 4, 0.0, 1.0, lists)
    assert [f.shape for f in r["full"]] == [(3, 3), (3, 0), (3, 1)]                 # 9 pairs of 4: 4 + 4 + 1
    assert r["cnt"].tolist() == [[3, 0, 3], [0, 0, 0], [1, 1, 0]] and r["flag"].tolist() == [0, 0, 0]
    assert np.isnan(r["full"][0][1]).all() and r["total"][0, 1] == 0 and not r["total"][1].any()
    assert r["ids"][0].tolist() == pos[[0, 4, 8]].tolist() and r["ids"][2].tolist() == [pos[9]]
    assert np.allclose(r["total"][0, 0], np.abs(r["full"][0][0]).sum())
    # the last entry alone: the one pair's own term
    Z, c = R.item_side(Gi, Bi, P, 3)
    w = np.concatenate([Gu[0], Tu[0]]).astype(np.float64)
    D, s, cp = R.row_terms(Z, c, w, pos[:9], neg[:9])
    A = (D * cp[:, None]).T @ D
    lam = np.trace(A) / 7
    want = Z[1] @ np.linalg.solve(A + lam * np.eye(7), s[8] * D[8])
    assert np.allclose(r["full"][0][0][2], want, rtol=1e-10)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 2e-4)])
def test_the_entries_sum_to_the_whole_gradient_and_large_damping_leaves_the_plain_dot(dtype, tol):
    Gi, Bi, P, Gu, Tu, ptr, pos, neg = _case(2, 2, 6, 4, [7, 12], 5, short=2)
    lists = np.array([[3, 9, 11], [0, 1, 2]])
    Z, c = R.item_side(Gi, Bi, P, 4)
    r = R.influence(Gi, Bi, P, Gu, Tu, ptr, pos, neg, 5, 1e-3, 0.5, lists, dtype)
    big = R.influence(Gi, Bi, P, Gu, Tu, ptr, pos, neg, 5, 0.0, 1e9, lists, dtype)
    for u in range(2):
        i, j = pos[ptr[u]:ptr[u + 1]], neg[ptr[u]:ptr[u + 1]]
        w = np.concatenate([Gu[u], Tu[u]]).astype(np.float64)
        D, s, cp = R.row_terms(Z, c, w, i, j)
        A = (D * cp[:, None]).T @ D
        lam = 2 * 1e-3 * len(i) + 0.5 * np.trace(A) / 10
        whole = Z[lists[u]] @ np.linalg.solve(A + lam * np.eye(10), (s[:, None] * D).sum(0))
        assert np.allclose(r["full"][u].sum(1), whole, rtol=tol, atol=tol * np.abs(whole).max())
        lam9 = 1e9 * np.trace(A) / 10                             # damp -> infinity: lambda infl(q, e) -> z_q . g_e
        ge = R.entry_sums((s[:, None] * D).T, 5).T                # [M, n]
        assert np.allclose(lam9 * big["full"][u].astype(np.float64), Z[lists[u]] @ ge.T, rtol=max(tol, 1e-6), atol=1e-6)
    assert r["full"][0].dtype == dtype


def test_the_cholesky_pair_and_the_flag():
    rs = np.random.RandomState(3)
    B = rs.standard_normal((9, 9))
    A = B @ B.T + 9 * np.eye(9)
    for dt, tol in ((np.float64, 1e-12), (np.float32, 1e-4)):
        L = R.cholesky(A.astype(dt))
        assert L.dtype == dt and np.allclose(L @ L.T, A, rtol=tol, atol=tol) and not np.triu(L, 1).any()
        X = R.solve(L, rs.standard_normal((9, 4)).astype(dt))
        assert X.dtype == dt
    rhs = rs.standard_normal((9, 4))
    assert np.allclose(R.solve(R.cholesky(A), rhs), np.linalg.solve(A, rhs), rtol=1e-10)
    assert R.cholesky(np.zeros((3, 3))) is None and R.cholesky(np.array([[1.0, 2.0], [2.0, 1.0]])) is None
    assert R.cholesky(np.array([[np.nan]])) is None and R.cholesky(np.array([[np.inf]])) is None
    # all-zero item rows with reg = 0: A = 0, lambda = 0 -- the row is flagged, its slots are empty
    Gi, Bi, P, Gu, Tu, ptr, pos, neg = _case(4, 2, 4, 0, [3, 3], 2)
    Gi[:] = 0
    r = R.influence(Gi, Bi, None, Gu, None, ptr, pos, neg, 2, 0.0, 1.0, np.array([[1, 2], [3, 4]]))
    assert r["flag"].tolist() == [1, 1] and not r["cnt"].any() and not r["total"].any() and r["full"][0].shape == (2, 0)
    assert R.top_entries(np.array([0.0, -0.0, 0.5, -0.0, 0.5], np.float32), 4).tolist() == [2, 4, 0, 1]      # -0 == +0, ties by position


def test_influence_predicts_the_fall_of_a_score_under_a_leave_one_entry_out_refit():
    """The claim, on the restatement alone.  A well-posed case: n = 8, 120 entries x 4 pairs, reg = 1e-3, damp = 0, the row fitted
    to its optimum by Newton in float64.  infl(q, e) against the actual fall of 20 scores when entry e's pairs leave the objective
    (same ridge 2 reg m) and the row is refitted to the new optimum: Pearson correlation >= 0.99 over all 20 x 120 values."""
    rs = np.random.RandomState(11)
    I, n, E, pe, reg = 200, 8, 120, 4, 1e-3
    Gi, Bi = (rs.standard_normal((I, n)) * 0.5).astype(np.float32), (rs.standard_normal(I) * 0.1).astype(np.float32)
    Z, c = R.item_side(Gi, Bi, None, 0)
    hist = rs.randint(I, size=E)
    pos, neg = np.repeat(hist, pe), rs.randint(I, size=E * pe)
    m = E * pe
    w = R.newton_fit(Z, c, pos, neg, reg * m, np.zeros(n))
    D, s, _ = R.row_terms(Z, c, w, pos, neg)
    assert np.abs(-(s[:, None] * D).sum(0) + 2 * reg * m * w).max() < 1e-10          # the optimum
    q = rs.choice(I, size=20, replace=False)
    ptr = np.array([0, m], np.int64)
    r = R.influence(Gi, Bi, None, w[None, :].astype(np.float64), None, ptr, pos, neg, pe, reg, 0.0, q[None, :])
    # (the restatement takes the row as float32 tables: here the float64 optimum is wanted, so the terms are formed directly)
    Dw, sw, cw = R.row_terms(Z, c, w, pos, neg)
    A = (Dw * cw[:, None]).T @ Dw + 2 * reg * m * np.eye(n)
    V = np.linalg.solve(A, Z[q].T)
    infl = R.entry_sums(((Dw @ V) * sw[:, None]).T, pe)                              # [20, E]
    assert np.allclose(infl, r["full"][0], rtol=1e-4, atol=1e-7)                      # the restatement on the float32-rounded row agrees
    fall = np.zeros((20, E))
    for e in range(E):
        keep = np.ones(m, bool)
        keep[e * pe:(e + 1) * pe] = False
        w_e = R.newton_fit(Z, c, pos, neg, reg * m, w, keep)
        fall[:, e] = Z[q] @ (w - w_e)
    corr = np.corrcoef(infl.reshape(-1), fall.reshape(-1))[0, 1]
    print("leave-one-entry-out: Pearson %.5f over %d values" % (corr, infl.size))
    assert corr >= 0.99


# ---- naming --------------------------------------------------------------------------------------------------------------------
def test_influence_file_names():
    assert ranking.INFLUENCE_FILES == {"influence": None, "influence-new-user-recs": None}
    for table in (ranking.RUN_FILES, ranking.ITEM_FILES, ranking.WARM_FILES, ranking.SHELF_FILES, ranking.STYLE_FILES):
        assert not set(ranking.INFLUENCE_FILES) & set(table)
    assert len(ranking.RUN_FILES) == 14
    d = os.path.join("res", "rec_results", "toy", "vbpr")
    tail = "batch_64-K_8-lr_0.001-reg_0.0.tsv"
    for f, kind, want in (("recs-3-" + tail, "influence", "influence-3-" + tail),
                          ("best-recs-2-" + tail, "influence", "best-influence-2-" + tail),
                          ("recs-3-" + tail, "influence-new-user-recs", "influence-new-user-recs-3-" + tail),
                          ("best-recs-2-" + tail, "influence-new-user-recs", "best-influence-new-user-recs-2-" + tail)):
        assert ranking.influence_file(os.path.join(d, f), kind) == os.path.join(d, want)
    for bad in ("sim-3-" + tail, "new-user-recs-3-" + tail, "because-3-" + tail, "influence-3-" + tail):
        with pytest.raises(ValueError):
            ranking.influence_file(os.path.join(d, bad), "influence")
    with pytest.raises(ValueError):
        ranking.influence_file(os.path.join(d, "recs-3-" + tail), "because")


# ---- command line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["--rec", "acf", "--influence", "3"],
    ["--rec", "attentive_fashion", "--influence", "3"],
    ["--rec", "vbpr", "--influence", "-1"],
    ["--rec", "vbpr", "--influence", "33"],
    ["--rec", "vbpr", "--influence", "3", "--influence_damp", "-0.5"],
    ["--rec", "vbpr", "--influence", "3", "--influence_damp", "inf"],
    ["--rec", "vbpr", "--influence", "3", "--influence_damp", "nan"],
    ["--rec", "vbpr", "--influence", "3", "--influence_damp", "0"],                   # reg defaults to 0
    ["--rec", "bprmf", "--influence", "3", "--influence_damp", "0", "--reg", "0"],
], ids=lambda a: " ".join(a))
def test_parse_args_rejects(argv, capsys):
    with pytest.raises(SystemExit):
        train_rec.parse_args(argv)
    assert "influence" in capsys.readouterr().err


def test_parse_args_defaults_and_the_single_gpu_rule():
    for rec in ("bprmf", "vbpr", "grad_fashion"):
        a = train_rec.parse_args(["--rec", rec])
        assert a.influence == 0 and a.influence_damp == 1.0
        a = train_rec.parse_args(["--rec", rec, "--influence", "32"])
        assert a.influence == 32
    assert train_rec.parse_args(["--rec", "acf"]).influence == 0                               # off: every model trains as before
    a = train_rec.parse_args(["--rec", "vbpr", "--influence", "5", "--influence_damp", "0", "--reg", "0.01"])
    assert (a.influence, a.influence_damp) == (5, 0.0)
    a = train_rec.parse_args(["--rec", "vbpr", "--influence", "5", "--because", "4", "--feat_explain", "4", "--diversify", "0.5"])
    assert (a.influence, a.because, a.feat_explain, a.diversify) == (5, 4, 4, 0.5)             # combines freely
    with pytest.raises(NotImplementedError, match="influence"):
        train_rec.train(["--rec", "vbpr", "--influence", "3", "--world_size", "2"])
    with pytest.raises(ValueError, match="influence"):
        train_rec.train(["--rec", "vbpr", "--influence", "3", "--top_k", "1025"])


def test_models_whose_score_is_not_linear_in_the_row_name_their_own_flag():
    from fashionvisualexpl_recommend_amd import models
    for cls, flag in ((models.ACF, "--acf_explain"), (models.AttentiveFashion, "--af_explain")):
        obj = cls.__new__(cls)                                         # (no engine is needed to refuse)
        with pytest.raises(NotImplementedError, match=flag):
            obj.influence([0], [1])


# ---- writer --------------------------------------------------------------------------------------------------------------------
def test_write_influence_rows():
    ids = np.array([[4, 9], [7, 3]], np.int64)
    vals = np.array([[1.5, -0.0], [3.0, 0.25]], np.float32)
    hist = np.array([[[8, 2, -1], [-1, -1, -1]], [[5, 6, 1], [2, -1, -1]]], np.int64)
    infl = np.array([[[0.75, -0.25, 0], [0, 0, 0]], [[1.0, 0.5, -0.25], [0.0, 0, 0]]], np.float32)
    total = np.array([[1.0, 0.0], [4.0, 0.0]], np.float32)
    out = io.StringIO()
    ranking.write_influence(out, ["u a", 8], ids, vals, hist, infl, total)
    assert out.getvalue() == ("u a\t4\t1.5\t0\t8\t0.75\t0.75\nu a\t4\t1.5\t1\t2\t-0.25\t-0.25\n"
                              "u a\t9\t-0.0\t-1\t-1\t0.0\t0.0\n"                               # no entry: the pair is still named
                              "8\t7\t3.0\t0\t5\t1.0\t0.25\n8\t7\t3.0\t1\t6\t0.5\t0.125\n8\t7\t3.0\t2\t1\t-0.25\t-0.0625\n"
                              "8\t3\t0.25\t0\t2\t0.0\t0.0\n")                                  # total 0: share 0
    plain = io.StringIO()
    ranking.write_ranked(plain, ["u a", 8], ids, vals)
    heads = [l.rsplit("\t", 4)[0] for l in out.getvalue().splitlines()]
    assert list(dict.fromkeys(heads)) == plain.getvalue().splitlines()
    third = np.float32(1.0) / np.float32(3.0)                                                  # share is a float32 quotient
    one = io.StringIO()
    ranking.write_influence(one, [1], ids[:1, :1], vals[:1, :1], np.array([[[6]]]), np.array([[[1.0]]], np.float32), np.array([[3.0]], np.float32))
    assert one.getvalue() == "1\t4\t1.5\t0\t6\t1.0\t%s\n" % str(third)
    empty = io.StringIO()
    ranking.write_influence(empty, [1], ids[:1], vals[:1], np.zeros((1, 2, 0), np.int64), np.zeros((1, 2, 0), np.float32), np.zeros((1, 2), np.float32))
    assert empty.getvalue() == "1\t4\t1.5\t-1\t-1\t0.0\t0.0\n1\t9\t-0.0\t-1\t-1\t0.0\t0.0\n"


# ---- pairs -> lists ------------------------------------------------------------------------------------------------------------
def _stub(calls, L, maps=False):
    """An entry that answers slot (r, q) with item = 1000 r + q, infl = the slot's list entry, total = the first element of the
    row, cnt = the row's pairs, and records what it was given."""
    def entry(Gu, Tu, ptr, pos, neg, li):
        assert li.dtype == torch.int32 and li.is_contiguous() and ptr.dtype == torch.int64 and pos.dtype == neg.dtype == torch.int32
        n, K = li.shape
        assert Gu.shape[0] == n and Tu is None and ptr.numel() == n + 1
        calls.append((li.numpy().copy(), ptr.numpy().copy(), pos.numpy().copy(), neg.numpy().copy(), Gu.numpy().copy()))
        res = {"item": (1000 * torch.arange(n)[:, None, None] + torch.arange(K)[None, :, None] + torch.zeros(1, 1, L)).to(torch.int32),
               "infl": li[:, :, None].float() + torch.zeros(1, 1, L),
               "total": Gu[:, :1].expand(n, K).contiguous(), "cnt": (ptr[1:] - ptr[:-1])[:, None].expand(n, K).to(torch.int32),
               "flag": torch.zeros(n, dtype=torch.int32)}
        if maps:
            res["full"] = torch.zeros((n, K, 4)) + torch.arange(n)[:, None, None]
        return res
    return entry


def test_pairs_become_lists_by_runs_of_equal_users_with_one_draw_per_run():
    lists = [[5, 6, 5], [], [7], [1, 2, 3, 3]]
    users = [3, 3, 0, 0, 0, 3, 2]
    items = [10, 11, 12, 13, 14, 15, 16]
    drawn = []

    def draw(hists):                                             # two pairs per history item: (item, item + 100)
        drawn.append([list(h) for h in hists])
        ptr = np.cumsum([0] + [2 * len(h) for h in hists]).astype(np.int64)
        pos = np.array([i for h in hists for i in h for _ in range(2)], np.int32)
        return ptr, pos, pos + 100

    rows = lambda ids: (torch.as_tensor(np.asarray(ids, np.float32))[:, None] * torch.ones(1, 3), None)
    calls = []
    hist, infl, total, cnt, full = ranking.influence_rows(_stub(calls, 2, True), users, items, lists, 2, "cpu", draw, rows, maps=True)
    assert len(calls) == 1 and drawn == [[[1, 2, 3, 3], [5, 6, 5], [1, 2, 3, 3], [7]]]             # a user's second run: drawn again
    li, ptr, pos, neg, Gu = calls[0]
    assert li.tolist() == [[10, 11, -1], [12, 13, 14], [15, -1, -1], [16, -1, -1]]
    assert ptr.tolist() == [0, 8, 14, 22, 24] and pos[:8].tolist() == [1, 1, 2, 2, 3, 3, 3, 3] and (neg == pos + 100).all()
    assert Gu[:, 0].tolist() == [3.0, 0.0, 3.0, 2.0]                                               # the rows of the lists' users
    assert hist.dtype == np.int64 and hist.shape == (7, 2) and infl.shape == (7, 2) and total.shape == (7,) and cnt.shape == (7,)
    assert hist[:, 0].tolist() == [0, 1, 1000, 1001, 1002, 2000, 3000] and infl[:, 1].tolist() == [float(i) for i in items]
    assert total.tolist() == [3.0, 3.0, 0.0, 0.0, 0.0, 3.0, 2.0] and cnt.tolist() == [8, 8, 6, 6, 6, 8, 2]
    assert full.shape == (7, 4) and full[:, 0].tolist() == [0, 0, 1, 1, 1, 2, 3]
    # a run of more than 1024 pairs: its lists share the run's one draw
    calls.clear(); drawn.clear()
    out = ranking.influence_rows(_stub(calls, 1), [2] * 1030 + [0], list(range(1031)), lists, 1, "cpu", draw, rows)
    assert len(out) == 4 and drawn == [[[7], [5, 6, 5]]]
    li, ptr, pos, neg, Gu = calls[0]
    assert li.shape == (3, 1024) and ptr.tolist() == [0, 2, 4, 10] and pos.tolist() == [7, 7, 7, 7, 5, 5, 6, 6, 5, 5]
    assert Gu[:, 0].tolist() == [2.0, 2.0, 0.0] and out[3].tolist() == [2] * 1030 + [6]
    calls.clear()
    out = ranking.influence_rows(_stub(calls, 3), [], [], lists, 3, "cpu", draw, rows, maps=True)
    assert not calls and out[0].shape == (0, 3) and out[2].shape == (0,) and out[4].shape == (0, 0)
    with pytest.raises(ValueError):
        ranking.influence_rows(_stub(calls, 3), [0, 0], [1], lists, 3, "cpu", draw, rows)
