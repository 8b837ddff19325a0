"""Audiences without a GPU: the binding and the library's exports, ranking.owners_of and the ITEM_FILES naming table, the command
line, the lists and the files of BPRMF.audience / VBPR.audience_new / Evaluator.store_audience[_new] over a stub engine (in the
manner of tests/test_similar_cpu.py: determined rows answered with the unique list, every other row flagged and POISONED, so a
flagged row's kernel output must not be read), and tests/audience_ref.py against a plain double loop."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import audience_ref as A
import new_items_ref as N
import topk_ref as tr
from fashionvisualexpl_recommend_amd import _ffi, models, ranking, train_rec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = "2-batch_64-D_8-K_16-lr_0.001-reg_0.0.tsv"


# ---- binding and exports -------------------------------------------------------------------------------------------------------
def test_the_binding_declares_and_the_library_exports_the_two_entries():
    header = open(os.path.join(REPO, "include", "bprx.h")).read()
    lib = _ffi.lib()
    for name, nargs in (("bprx_audience_block", 7), ("bprx_topk_rows_masked", 11)):
        assert name in _ffi.EXPORTS
        assert re.search(r"BPRX_API int %s\(" % name, header), name
        fn = getattr(lib, name)                               # AttributeError: the library does not export it
        assert len(fn.argtypes) == nargs
    assert "#define BPRX_ABI_VERSION 6" in header and _ffi.ABI_VERSION == 6 and lib.bprx_abi_version() == 6
    # a NULL handle is rejected before anything is read
    assert lib.bprx_audience_block(None, None, 0, 0, 0, None, None) == _ffi.E_INVALID
    assert lib.bprx_topk_rows_masked(None, 0, 1, None, None, None, 1, None, None, None, None) == _ffi.E_INVALID


# ---- owners --------------------------------------------------------------------------------------------------------------------
def test_owners_of_against_a_double_loop():
    rs = np.random.RandomState(2)
    U, I = 23, 11
    tl = [rs.randint(0, I, size=rs.randint(0, 7)).tolist() for _ in range(U)]
    tl[4] = [3, 3, 9, 3]                                      # repeats: user 4 owns item 3 once
    tl[7] = []
    tl = [[i for i in l if i != 6] for l in tl]               # nobody owns item 6
    tl[9] = tl[9] + [I, -1, I + 5]                            # ids outside the catalogue have no row
    got = ranking.owners_of(tl, I)
    assert len(got) == I
    for i in range(I):
        want = [u for u in range(U) if any(j == i for j in tl[u])]
        assert got[i].tolist() == want and got[i].dtype == np.int64, i
    assert got[6].size == 0 and got[3].tolist().count(4) == 1
    assert [g.tolist() for g in got] == A.owners(tl, I)
    assert ranking.owners_of([], 3)[2].size == 0 and len(ranking.owners_of([], 3)) == 3 and ranking.owners_of(tl, 0) == []
    assert [g.tolist() for g in ranking.owners_of([[0], [0]], 1)] == [[0, 1]]
    # the mask of a block of items, as the model builds it
    ptr, items = ranking.lists_to_csr(got[2:5], "cpu")
    assert ptr.tolist() == np.cumsum([0] + [g.size for g in got[2:5]]).tolist()
    assert items.tolist()[:int(ptr[-1])] == [u for g in got[2:5] for u in g.tolist()]


# ---- the reference against a double loop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("feat_dtype", ["fp32", "bf16"])
def test_audience_ref_against_a_double_loop(feat_dtype):
    from oracle import oracle as orc
    rs = np.random.RandomState(3)
    U, I, k, d, D, n = 5, 4, 3, 2, 6, 3
    t = dict(Gu=rs.standard_normal((U, k)), Gi=rs.standard_normal((I, k)), Bi=rs.standard_normal(I), Tu=rs.standard_normal((U, d)),
             F=rs.standard_normal((I, D)), E=rs.standard_normal((D, d)), Bp=rs.standard_normal(D))
    t = {nm: v.astype(np.float32) for nm, v in t.items()}
    Fn = rs.standard_normal((n, D)).astype(np.float32)
    if feat_dtype == "bf16":
        t["F"], Fn = orc.bf16_round(t["F"]), orc.bf16_round(Fn)
    E, Bp = (orc.bf16_round(t[nm]) if feat_dtype == "bf16" else t[nm] for nm in ("E", "Bp"))
    f = lambda x: float(x)

    def visual(frow, u):
        return sum(f(t["Tu"][u, x]) * sum(f(frow[c]) * f(E[c, x]) for c in range(D)) for x in range(d)) + \
            sum(f(frow[c]) * f(Bp[c]) for c in range(D))

    want = np.array([[f(t["Bi"][q]) + sum(f(t["Gu"][u, x]) * f(t["Gi"][q, x]) for x in range(k)) + visual(t["F"][q], u)
                      for u in range(U)] for q in range(I)])
    want_new = np.array([[visual(Fn[j], u) for u in range(U)] for j in range(n)])
    mf = np.array([[f(t["Bi"][q]) + sum(f(t["Gu"][u, x]) * f(t["Gi"][q, x]) for x in range(k)) for u in range(U)] for q in range(I)])
    got, got_new = A.scores(t, feat_dtype), A.scores(t, feat_dtype, F=Fn)
    assert got.shape == (I, U) and got.dtype == np.float64 and np.allclose(got, want, rtol=1e-12, atol=1e-14)
    assert got_new.shape == (n, U) and np.allclose(got_new, want_new, rtol=1e-12, atol=1e-14)
    assert np.allclose(A.scores({nm: t[nm] for nm in ("Gu", "Gi", "Bi")}), mf, rtol=1e-13, atol=1e-15)     # BPRMF
    assert np.array_equal(got, A.user_major(t, feat_dtype).T)
    assert np.array_equal(got_new, N.scores(t["Tu"], Fn, t["E"], t["Bp"], 0, U, feat_dtype).T)      # the existing restatement, transposed
    g32 = A.scores(t, feat_dtype, torch.float32)
    assert g32.dtype == np.float32 and np.abs(g32 - want).max() < 1e-4
    # owners and the masked lists: value descending, id ascending, -1 / -inf past the non-owners
    own = [[0, 3], [], [0, 1, 2, 3, 4], [1, 2, 4]]
    S = want.copy()
    S[0, 1] = S[0, 2] = 7.0                                   # equal values: the lower id first
    ids, vals = A.lists(S, own, 3)
    for q in range(I):
        live = sorted((u for u in range(U) if u not in own[q]), key=lambda u: (-S[q, u], u))[:3]
        assert ids[q, :len(live)].tolist() == live and (ids[q, len(live):] == -1).all()
        assert vals[q, :len(live)].tolist() == [S[q, u] for u in live] and np.isneginf(vals[q, len(live):]).all()
    assert ids[0, :2].tolist() == [1, 2] and (ids[2] == -1).all() and ids[3].tolist() == [*sorted([0, 3], key=lambda u: -S[3, u]), -1]
    assert A.lists(S, own, 9)[0].shape == (I, U)


# ---- file names ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("best", ["", "best-"])
def test_item_files_map_to_their_names(best):
    assert sorted(ranking.ITEM_FILES) == ["audience", "new-audience"]
    assert not set(ranking.ITEM_FILES) & set(ranking.RUN_FILES) and len(ranking.RUN_FILES) == 14
    for d in ("", os.path.join("res", "rec_results", "toy", "vbpr")):
        base = os.path.join(d, best + "recs-" + TAIL)
        assert ranking.item_file(base, "audience") == os.path.join(d, best + "audience-" + TAIL)
        assert ranking.item_file(base, "new-audience") == os.path.join(d, best + "new-audience-" + TAIL)
        for kind in ranking.ITEM_FILES:
            with pytest.raises(ValueError):
                ranking.run_file(base, kind)                  # the user-side table does not know them
        for kind in ranking.RUN_FILES:
            with pytest.raises(ValueError):
                ranking.item_file(base, kind)
    assert ranking.item_file(best + "recs-host.tsv", "audience") == best + "audience-host.tsv"


def test_a_path_that_is_no_list_file_raises():
    d = os.path.join("res", "toy")
    for bad in ("results-metrics-x.pkl", "expl-" + TAIL, "sim-" + TAIL, "new-recs-" + TAIL, "new-user-recs-" + TAIL, "div-recs-" + TAIL,
                "best-expl-" + TAIL, "best-" + TAIL, "my-recs-" + TAIL, "recs" + TAIL, "bestrecs-" + TAIL, "",
                "audience-" + TAIL, "best-audience-" + TAIL, "new-audience-" + TAIL):
        for path in (bad, os.path.join(d, bad)):
            for kind in ranking.ITEM_FILES:
                with pytest.raises(ValueError):
                    ranking.item_file(path, kind)
    with pytest.raises(ValueError):
        ranking.item_file(os.path.join("recs-dir", "x.tsv"), "audience")     # the file's name decides, not its directory's
    with pytest.raises(ValueError):
        ranking.item_file("recs-" + TAIL, "best-audience")                   # no such kind


# ---- command line --------------------------------------------------------------------------------------------------------------
def _ids_file(tmp_path, text, name="ids.txt"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_parse_args_rejects(tmp_path, capsys):
    good = _ids_file(tmp_path, "3\n0\n\n3\n")
    for argv in (["--rec", "acf", "--audience", "5"],
                 ["--rec", "attentive_fashion", "--audience", "5"],
                 ["--rec", "vbpr", "--audience", "-1"],
                 ["--rec", "vbpr", "--audience", "1025"],
                 ["--rec", "bprmf", "--audience_items", good],                                   # without --audience
                 ["--rec", "bprmf", "--audience", "0", "--audience_items", good],
                 ["--rec", "bprmf", "--audience", "5", "--audience_items", _ids_file(tmp_path, "3\n-2\n", "neg.txt")],
                 ["--rec", "bprmf", "--audience", "5", "--audience_items", _ids_file(tmp_path, "3\nx\n", "word.txt")],
                 ["--rec", "bprmf", "--audience", "5", "--audience_items", str(tmp_path / "missing.txt")]):
        with pytest.raises(SystemExit):
            train_rec.parse_args(argv)
        assert "audience" in capsys.readouterr().err, argv
    # an id outside the catalogue: known once the data is loaded, rejected the same way
    args = train_rec.parse_args(["--rec", "bprmf", "--audience", "5", "--audience_items", good])
    train_rec.check_audience_items(args, 4)
    with pytest.raises(SystemExit):
        train_rec.check_audience_items(args, 3)
    assert "audience" in capsys.readouterr().err
    assert train_rec.read_audience_items(good) == [3, 0, 3] and train_rec.read_audience_items(good, 4) == [3, 0, 3]
    with pytest.raises(ValueError, match="audience"):
        train_rec.read_audience_items(good, 3)


def test_parse_args_defaults_and_world_size(tmp_path):
    for rec in ("bprmf", "vbpr", "grad_fashion", "acf", "attentive_fashion"):
        a = train_rec.parse_args(["--rec", rec])
        assert a.audience == 0 and a.audience_items is None   # off
    train_rec.check_audience_items(train_rec.parse_args(["--rec", "acf"]), 3)
    for rec in ("bprmf", "vbpr", "grad_fashion"):
        assert train_rec.parse_args(["--rec", rec, "--audience", "1024"]).audience == 1024
    a = train_rec.parse_args(["--rec", "vbpr", "--dtype", "fp8", "--audience", "1", "--audience_items", _ids_file(tmp_path, "7\n")])
    assert a.audience == 1 and a.audience_items.endswith("ids.txt")
    with pytest.raises(NotImplementedError, match="audience"):
        train_rec.train(["--rec", "vbpr", "--audience", "5", "--world_size", "2"])


# ---- lists and files over a stub engine ----------------------------------------------------------------------------------------
class _StubEngine:
    """The engine calls audience / audience_new make, on the CPU: float32 scores from audience_ref, the top-K entries of
    tests/test_ranking_cpu.py (mask IN the scores; undetermined rows come back flagged with idx -1 / val nan)."""
    device = "cpu"

    def __init__(self, **kw):
        self.kw, self.blocks, self.new_blocks, self.flags = kw, [], [], []
        self.feat_dtype = kw.get("feat_dtype", "fp32")

    def bind(self, **t):
        self.t = t
        return self

    def csr(self, lists):
        return [[int(u) for u in l] for l in lists]

    def _new_table(self, F):
        return torch.as_tensor(np.asarray(F, np.float32))

    def project_rows(self, F):
        return torch.from_numpy(N.projection(F.numpy(), self.t["E"], self.t["Bp"], "fp32", torch.float32))

    def audience_block(self, q0, q1, P=None):
        if P is None:
            self.blocks.append((q0, q1))
            return torch.from_numpy(A.scores(self.t, "fp32", torch.float32)[q0:q1].copy())
        self.new_blocks.append((q0, q1))
        d = P.shape[1] - 1
        return (P[q0:q1, :d] @ torch.as_tensor(self.t["Tu"]).T + P[q0:q1, d][:, None]).contiguous()

    def _topk(self, s, own, k):
        n, U = s.shape
        for r, l in enumerate(own):
            s[r, l] = -np.inf
        idx, val, flag = np.full((n, k), -1, np.int32), np.full((n, k), np.nan, np.float32), np.ones(n, np.int32)
        for r in range(n):
            if tr.classify(s[r], k, U - len(set(own[r]))) == tr.DETERMINED:
                idx[r] = tr.unique_topk(s[r], k)
                val[r], flag[r] = s[r][idx[r]], 0
        self.flags.append(flag.copy())
        return torch.from_numpy(idx), torch.from_numpy(val), torch.from_numpy(flag)

    def topk_rows_masked(self, scores, own, k):
        assert len(own) == scores.shape[0]
        return self._topk(scores.numpy(), own, k)

    def topk_rows(self, scores, k):
        return self._topk(scores.numpy(), [[] for _ in range(scores.shape[0])], k)


U_USERS, I_ITEMS, ALMOST = 20, 9, 4                           # item ALMOST is owned by all but three users
NON_OWNERS = [2, 11, 17]


def _data():
    rs = np.random.RandomState(12)
    tl = [rs.choice([i for i in range(I_ITEMS) if i not in (ALMOST, 6)], size=rs.randint(0, 4), replace=False).tolist()
          for _ in range(U_USERS)]                            # nobody owns item 6
    for u in range(U_USERS):
        if u not in NON_OWNERS:
            tl[u] = tl[u] + [ALMOST]
    tl[5] = tl[5] + tl[5]                                     # a list that names its items twice
    return Namespace(num_users=U_USERS, num_items=I_ITEMS, training_list=tl, validation_list=[], test_list=[],
                     params=Namespace(batch_eval=128))


def _model(monkeypatch, cls="bprmf", **over):
    monkeypatch.setattr(models, "Engine", _StubEngine)
    rs = np.random.RandomState(11)
    Gu = rs.standard_normal((U_USERS, 6)).astype(np.float32)
    Tu = rs.standard_normal((U_USERS, 3)).astype(np.float32)
    Gu[8], Tu[8] = Gu[3], Tu[3]                               # twin users: equal scores for every item, lists numpy has to order
    p = dict(epochs=1, batch_size=16, embed_k=6, embed_d=3, lr=0.001, reg=0, top_k=3, dataset="toy", rec=cls, optimizer="sgd",
             init_seed=0)
    p.update(over)
    data = _data()
    if cls == "bprmf":
        m = models.BPRMF(data, Namespace(**p), init={"Gu": Gu})
    else:
        m = models.VBPR(data, Namespace(**p), init={"Gu": Gu, "Tu": Tu}, features=rs.standard_normal((I_ITEMS, 10)).astype(np.float32))
    return m, data


def _reference_lists(S, own, k):
    """numpy_topk on every masked float32 row, -1 where the masked value is -inf: the list whether or not the kernel flags."""
    sc = A.masked(S, own)
    kk = min(k, sc.shape[1])
    ids = np.stack([ranking.numpy_topk(sc[r], k)[:kk] for r in range(sc.shape[0])]).astype(np.int64)
    vals = np.take_along_axis(sc, ids, axis=1)
    ids[np.isneginf(vals)] = -1
    return ids, vals, sc


def _text(labels, ids, vals):
    return "".join("%s\t%s\t%s\n" % (lab, ids[r, q], str(vals[r, q])) for r, lab in enumerate(labels)
                   for q in range(ids.shape[1]) if ids[r, q] >= 0)


@pytest.mark.parametrize("block", [4, 1, 4096])
@pytest.mark.parametrize("k", [5, U_USERS, 64])
def test_audience_lists(monkeypatch, k, block):
    m, data = _model(monkeypatch, audience=k)
    assert m.audience_k == k
    m.evaluator.user_block = block
    own = A.owners(data.training_list, I_ITEMS)
    assert [u for u in range(U_USERS) if u not in own[ALMOST]] == NON_OWNERS and own[6] == []
    S = A.scores(m.engine.t, "fp32", torch.float32)
    ids, vals = m.audience()
    wid, wval, sc = _reference_lists(S, own, k)
    kk = min(k, U_USERS)
    assert ids.shape == vals.shape == (I_ITEMS, kk) and ids.dtype == np.int64 and vals.dtype == np.float32
    assert np.array_equal(ids, wid) and np.array_equal(vals.view(np.uint32), wval.view(np.uint32)) and not np.isnan(vals).any()
    rid, rval = A.lists(S, own, k)                            # the same values rank by rank; the same ids up to the order of equals
    assert np.array_equal(vals.view(np.uint32), rval.view(np.uint32))
    assert all(sorted(ids[r].tolist()) == sorted(rid[r].tolist()) for r in range(I_ITEMS))
    for i in range(I_ITEMS):                                  # an owner is never in an audience
        assert not set(ids[i][ids[i] >= 0].tolist()) & set(own[i]), i
        assert (ids[i] >= 0).sum() == min(kk, U_USERS - len(own[i]))
    assert ids[ALMOST, :3].tolist() == sorted(NON_OWNERS, key=lambda u: -S[ALMOST, u])
    assert (ids[ALMOST, 3:] == -1).all() and np.isneginf(vals[ALMOST, 3:]).all()
    step = min(block, I_ITEMS)
    assert m.engine.blocks == [(b, min(b + step, I_ITEMS)) for b in range(0, I_ITEMS, step)]
    flag = np.concatenate(m.engine.flags)
    assert flag[ALMOST] == 1                                  # fewer than k non-owners: through numpy
    if k == 5:
        assert 0 < flag.sum() < I_ITEMS                       # both kinds of row
    else:
        assert flag.all()                                     # the twins meet in every full row / k > U
    # an explicit id list, any order, with repeats: the blocks that hold the ids, those rows, in the order asked for
    m.engine.blocks.clear()
    pick = [8, ALMOST, 0, 0, 6]
    i2, v2 = m.audience(pick, k=k)
    assert m.engine.blocks == sorted({(q // step * step, min(q // step * step + step, I_ITEMS)) for q in pick})
    assert np.array_equal(i2, wid[pick]) and np.array_equal(v2.view(np.uint32), wval[pick].view(np.uint32))
    assert m.audience([], k=k)[0].shape == (0, kk)
    i3, _ = m.audience([6], k=3)                              # k: the call's, not the run's
    assert i3.shape == (1, 3) and (i3 >= 0).all()
    for bad in ([I_ITEMS], [-1]):
        with pytest.raises(ValueError, match="audience"):
            m.audience(bad)
    m2, _ = _model(monkeypatch)                               # the flag off: top_k users
    assert m2.audience_k == 0 and m2.audience()[0].shape == (I_ITEMS, 3)


@pytest.mark.parametrize("block", [4, 1])
def test_audience_new_lists(monkeypatch, block):
    m, data = _model(monkeypatch, "vbpr", audience=5)
    m.evaluator.user_block = block
    rs = np.random.RandomState(13)
    raw = rs.standard_normal((7, 10)).astype(np.float32)
    t = m.engine.t
    S = A.scores(t, "fp32", torch.float32, F=raw / np.float32(m.feat_norm))
    for k in (None, 5, U_USERS, 64):
        m.engine.new_blocks.clear()
        ids, vals = m.audience_new(raw, k)
        kq = 5 if k is None else k
        wid, wval, _ = _reference_lists(S, [[]] * 7, kq)
        assert ids.shape == (7, min(kq, U_USERS)) and (ids >= 0).all()                      # nothing is masked
        assert np.array_equal(ids, wid) and np.allclose(vals, wval, rtol=1e-5, atol=1e-6)
        assert m.engine.new_blocks == [(b, min(b + block, 7)) for b in range(0, 7, block)]
    assert m.audience_new(raw[:0], 5)[0].shape == (0, 5)


def test_store_audience_bytes(monkeypatch, tmp_path):
    m, data = _model(monkeypatch, "vbpr", audience=5)
    own = A.owners(data.training_list, I_ITEMS)
    S = A.scores(m.engine.t, "fp32", torch.float32)
    wid, wval, _ = _reference_lists(S, own, 5)
    want = _text(range(I_ITEMS), wid, wval)
    path = str(tmp_path / "audience-1-x.tsv")
    m.evaluator.store_audience(path)
    assert open(path).read() == want
    rows = [l.split("\t") for l in want.splitlines()]
    assert all(len(r) == 3 for r in rows) and [r[1] for r in rows if r[0] == str(ALMOST)] == [str(u) for u in wid[ALMOST, :3]]
    assert len(rows) == I_ITEMS * 5 - 2 and "-1" not in {r[1] for r in rows}                # the two empty slots are not written
    pick = [7, ALMOST, 7]
    m.evaluator.store_audience(path, pick)
    assert open(path).read() == _text(pick, wid[pick], wval[pick])
    # new items: rows 'j u score', j = the row of the table
    raw = np.random.RandomState(14).standard_normal((4, 10)).astype(np.float32)
    nid, nval = m.audience_new(raw)
    m.evaluator.store_audience_new(path, raw)
    assert open(path).read() == _text(range(4), nid, nval) and len(open(path).readlines()) == 20
    # what train() writes: audience-* next to recs-*, best-audience-* next to best-recs-*; with new items new-audience-* too;
    # the ids of --audience_items; nothing with the flag off
    np.save(str(tmp_path / "new.npy"), raw)
    ids_file = _ids_file(tmp_path, "7\n%d\n7\n" % ALMOST)
    for f in ("recs-2-x.tsv", "best-recs-1-x.tsv"):
        m._store_audience(str(tmp_path / f))
        assert open(str(tmp_path / f.replace("recs-", "audience-", 1))).read() == want
        assert not os.path.exists(str(tmp_path / f.replace("recs-", "new-audience-", 1)))
    m.params.new_items, m.params.audience_items = [str(tmp_path / "new.npy")], ids_file
    m._store_audience(str(tmp_path / "recs-3-x.tsv"))
    assert open(str(tmp_path / "audience-3-x.tsv")).read() == _text(pick, wid[pick], wval[pick])
    assert open(str(tmp_path / "new-audience-3-x.tsv")).read() == _text(range(4), nid, nval)
    with pytest.raises(ValueError):
        m._store_audience(str(tmp_path / "sim-3-x.tsv"))
    off, _ = _model(monkeypatch)
    off._store_audience(str(tmp_path / "recs-9-x.tsv"))
    assert off.audience_k == 0 and not os.path.exists(str(tmp_path / "audience-9-x.tsv"))
