"""bprx_topk at its edges, every row judged by the numpy classifier of tests/topk_ref.py (pinned on the CPU by
tests/test_topk_ref_cpu.py), and the Evaluator's device paths over the same families.

Rows (topk_ref.FAMILIES): distinct normals; a +0.0 / -0.0 pair inside the list, across its boundary (both index orders) and
below it; distinct denormals; one and two +inf; a natural -inf; five-level scores; train masks that leave exactly K and K - 1
items; a repeated train entry.  Shapes: I in {70, 300, 1030} (I < 256; more than one 256-thread sweep; just above 1024) times
K in {1, 2, 5, 64, 257, 1024}, which includes K > I three times and K = 1024 with I = 1030 / 300.  One launch of 104 rows per
pair.

  determined rows   flag 0, idx the unique answer, val bit-equal to the masked row at idx (the sign of a zero survives)
  must-flag rows    flag 1 (every K > I row; those also carry -1 / +0.0 from entry I on)
  fewer than K unmasked items: flag 1 (the header's contract; the classifier alone would accept either)
  the score buffer is the masked matrix afterwards, bit for bit; sync_check is clean.

+0.0 == -0.0 for numpy's argsort, which the reference (Evaluator.py:234), the host path and the redo of flagged rows use: a
selection by the bare bit image ranks +0.0 strictly above -0.0, leaves such rows unflagged and writes a list numpy does not."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import topk_ref as tr
from fashionvisualexpl_recommend_amd.evaluator import Evaluator

pytestmark = pytest.mark.gpu


def _bprmf(U, I):
    from fashionvisualexpl_recommend_amd.engine import Engine
    e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=4, optimizer="sgd", max_batch=8)
    return e.bind(Gu=np.zeros((U, 4), np.float32), Gi=np.zeros((I, 4), np.float32), Bi=np.zeros(I, np.float32))


def _csr(train):
    indptr = np.cumsum([0] + [len(l) for l in train]).astype(np.int64)
    items = np.array([i for l in train for i in l] or [0], np.int32)
    return torch.as_tensor(indptr, device="cuda"), torch.as_tensor(items, device="cuda")


@pytest.mark.parametrize("I,K", tr.SHAPES)
def test_topk_rows_against_the_classifier(I, K):
    sc, train, fams = tr.gen_rows(I, K)
    U = sc.shape[0]
    e = _bprmf(U, I)
    S = torch.as_tensor(sc, device="cuda").clone()
    idx, val, flag = e.topk(0, U, S, _csr(train), K)
    e.sync_check()
    bad = tr.check_launch(sc, train, fams, K, idx.cpu().numpy(), val.cpu().numpy(), flag.cpu().numpy(), S.cpu().numpy())
    e.close()
    assert not bad, "%d of %d rows, first: %s" % (len(bad), U, bad[:6])


# ---- the Evaluator end to end ------------------------------------------------------------------------------------------
class _ScoreModel:
    """A model whose score rows are a given matrix (the helper of tests/test_gpu_topk.py): score_block hands out a copy of
    the block, which the top-K kernel masks in place."""

    def __init__(self, data, scores):
        U, I = scores.shape
        self.data, self.scores = data, torch.as_tensor(scores, device="cuda")
        self.engine = _bprmf(U, I)
        self.engine.score_block = lambda u0, u1, out=None: self.scores[u0:u1].clone()

    def predict_block(self, u0, u1):
        return self.scores[u0:u1].cpu().numpy().copy()


U_E, I_E = 40, 300
# 16 rows per user block: the first block holds rows no kernel flags at K = 5, the second and third hold every tie family
E_FAMILIES = (("distinct", 4), ("zeros_below", 4), ("denormal", 3), ("inf_one", 2), ("neg_inf", 3),
              ("zeros_inside_pm", 3), ("zeros_inside_mp", 3), ("zeros_straddle_pm", 3), ("zeros_straddle_mp", 3), ("inf_two", 2),
              ("five_levels", 2),
              ("five_levels", 2), ("zeros_straddle_mp", 2), ("zeros_inside_pm", 1), ("distinct", 1), ("dup_train", 1),
              ("zeros_below", 1))


def _eval_data(n_test):
    """The 40 x 300 score matrix of the families above (laid out for K = 5) with its train lists; user u is given n_test(u)
    test items and one validation item, all outside its train list."""
    sc, train, fams = tr.gen_rows(I_E, 5, E_FAMILIES, seed=1)
    assert sc.shape == (U_E, I_E)
    rs = np.random.RandomState(11)
    test, val = [], []
    for u in range(U_E):
        free = rs.permutation(np.setdiff1d(np.arange(I_E), train[u]))
        n = n_test(u)
        test.append(free[:n].tolist())
        val.append(free[n:n + 1].tolist())
    data = Namespace(training_list=train, validation_list=val, test_list=test, num_users=U_E, num_items=I_E,
                     params=Namespace(batch_eval=128))
    return data, sc, train, fams


def test_eval_matrix_has_must_flag_rows_in_the_later_user_blocks():
    _, sc, train, fams = _eval_data(lambda u: 1)
    m = tr.mask(sc, train)
    cls = [tr.classify(m[u], 5, tr.n_unmasked(I_E, train[u])) for u in range(U_E)]
    assert set(cls[:16]) == {tr.DETERMINED}
    assert cls[16:32].count(tr.MUST_FLAG) >= 14 and cls[32:].count(tr.MUST_FLAG) >= 4 and tr.DETERMINED in cls[32:]
    e = _bprmf(U_E, I_E)
    for u0, u1 in ((0, 16), (16, 32), (32, 40)):            # the blocks as the Evaluator cuts them: u0 != 0 reads train_ptr[u0 + r]
        _, _, flag = e.topk(u0, u1, torch.as_tensor(sc[u0:u1], device="cuda").clone(), _csr(train), 5)
        assert flag.cpu().numpy().tolist() == [int(c == tr.MUST_FLAG) for c in cls[u0:u1]], (u0, u1)
    e.sync_check()
    e.close()


@pytest.mark.parametrize("K", [5, 400])
def test_store_recommendation_device_bytes_equal_host_bytes(tmp_path, K):
    data, sc, _, _ = _eval_data(lambda u: 1)
    ev = Evaluator(_ScoreModel(data, sc), data, K, user_block=16)
    dev_p, host_p = tmp_path / "dev.tsv", tmp_path / "host.tsv"
    ev.store_recommendation(str(dev_p))
    ev.model.engine.sync_check()
    ev.force_host = True
    ev.store_recommendation(str(host_p))
    got, want = dev_p.read_bytes(), host_p.read_bytes()
    assert len(want.splitlines()) == U_E * min(K, I_E)
    assert b"\t-0.0\n" in want and b"\tinf\n" in want        # the signed zero and the infinity reach the file
    assert got == want


@pytest.mark.parametrize("most", [32, 33])
def test_metrics_device_equal_host_with_32_and_33_held_out_items(most):
    """32 held-out items is the most the device kernel takes (EVMAX); one user with 33 sends the whole evaluation to the
    host (the -2 mark), which the caller must not notice."""
    n_test = lambda u: {20: 32, 35: most, 3: 0}.get(u, 1 + u % 3)
    data, sc, _, _ = _eval_data(n_test)
    ev = Evaluator(_ScoreModel(data, sc), data, 5, user_block=16)
    on_device = ev._metrics_device()
    assert (on_device is None) == (most == 33)
    got = ev.metrics()
    ev.model.engine.sync_check()
    ev.force_host = True
    want = ev.metrics()
    assert set(got) == set(want) and len(want) == 10
    for k in want:
        assert got[k] == pytest.approx(want[k], abs=1e-12), k


# ---- every device entry that lists a top-K against ranking.rank_rows_host of the same matrix ----------------------------------------
def _params(rec, K):
    return Namespace(dataset="toy", validation=True, batch_size=64, epochs=1, batch_eval=128, embed_k=4, embed_d=4, lr=0.05,
                     reg=1e-3, top_k=K, verbose=-1, restore_epochs=1, rec=rec, best_metric="ndcg", optimizer="sgd", init_seed=5,
                     dtype="fp32")


def _lists_store_recommendation(tmp_path, data, sc, train, K):
    ev = Evaluator(_ScoreModel(data, sc), data, K, user_block=16)
    ev.store_recommendation(str(tmp_path / "recs.tsv"))
    rows = [l.split("\t") for l in (tmp_path / "recs.tsv").read_text().splitlines()]
    kk = min(K, I_E)
    assert [int(r[0]) for r in rows] == [u for u in range(U_E) for _ in range(kk)]
    ids = np.array([int(r[1]) for r in rows]).reshape(U_E, kk)
    vals = np.array([np.float32(r[2]) for r in rows], np.float32).reshape(U_E, kk)      # (str of a float32 round-trips)
    return ev.model.engine, ids, vals, train


def _lists_new_users(tmp_path, data, sc, train, K):
    from fashionvisualexpl_recommend_amd.models import BPRMF
    m = BPRMF(data, _params("bprmf", K))
    S = torch.as_tensor(sc, device="cuda")
    m.evaluator.user_block = 16
    m.fold_in_users = lambda histories, **fold: (torch.zeros((len(histories), 4), dtype=torch.float32, device="cuda"), None)
    m.engine.score_rows_block = lambda Gu, Tu, r0, r1, out=None: S[r0:r1].clone()
    ids, vals = m.recommend_new_users(train)                   # the histories are the matrix's train lists: masked
    return m.engine, ids, vals, train


def _lists_new_items(tmp_path, data, sc, train, K):
    from fashionvisualexpl_recommend_amd import synth
    from fashionvisualexpl_recommend_amd.models import VBPR
    m = VBPR(data, _params("vbpr", K), features=synth.make_features(I_E, 32, seed=40))
    S = torch.as_tensor(sc, device="cuda")
    m.evaluator.user_block = 16
    m.engine.score_new_block = lambda u0, u1, P, out=None: S[u0:u1].clone()
    ids, vals = m.recommend_new(synth.make_features(I_E, 32, seed=41))       # 300 new items: the matrix's columns, nothing masked
    return m.engine, ids, vals, None


@pytest.mark.parametrize("K", [5, 400])
@pytest.mark.parametrize("entry", [_lists_store_recommendation, _lists_new_users, _lists_new_items],
                         ids=["store_recommendation", "recommend_new_users", "recommend_new"])
def test_every_device_entry_lists_as_rank_rows_host(tmp_path, entry, K):
    from fashionvisualexpl_recommend_amd.ranking import rank_rows_host
    data, sc, train, _ = _eval_data(lambda u: 1)
    eng, ids, vals, masks = entry(tmp_path, data, sc, train, K)
    eng.sync_check()
    eng.close()
    wid, wval = rank_rows_host(sc.copy(), masks, K)
    assert ids.shape == wid.shape == (U_E, min(K, I_E))
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert np.array_equal(ids, wid)
    assert np.array_equal(bits(vals), bits(wval))


class _ExplainedScoreModel(_ScoreModel):
    """_ScoreModel with the explain surfaces of VBPR (model.explain) and ACF (engine.acf_explain) stubbed: each records the
    (users, items) it is called with and explains nothing."""

    def __init__(self, data, scores):
        super().__init__(data, scores)
        self.calls = []
        self.engine.acf_train = self.engine.acf_eval = None
        self.engine.acf_explain = self._acf_explain

    def explain(self, users, items, top):
        self.calls.append((list(users), list(items)))
        n = len(users)
        return {"score": np.zeros(n, np.float32), "base": np.zeros(n, np.float32), "col": np.zeros((n, 0), np.int32),
                "contrib": np.zeros((n, 0), np.float32)}

    def _acf_explain(self, users, items, top=5, lists=None, csr=None, maps=False):
        self.calls.append((list(users), list(items)))
        n = len(users)
        return {"score": torch.zeros(n), "base": torch.zeros(n), "pos": torch.full((n, 1), -1, dtype=torch.int32)}


@pytest.mark.parametrize("K", [5, 400])
@pytest.mark.parametrize("writer", ["store_recommendation_acf", "store_recommendation_features"])
def test_explain_writers_receive_the_rec_files_pairs_block_by_block(tmp_path, writer, K):
    data, sc, _, _ = _eval_data(lambda u: 1)
    m = _ExplainedScoreModel(data, sc)
    ev = Evaluator(m, data, K, user_block=16)
    recs, expl, plain = tmp_path / "recs.tsv", tmp_path / "expl.tsv", tmp_path / "plain.tsv"
    getattr(ev, writer)(str(recs), str(expl), 3)
    ev.store_recommendation(str(plain))
    m.engine.sync_check()
    m.engine.close()
    assert recs.read_bytes() == plain.read_bytes()             # the rec file does not know that it is explained
    rows = [l.split("\t") for l in recs.read_text().splitlines()]
    kk = min(K, I_E)
    assert len(rows) == U_E * kk
    assert [len(c[0]) for c in m.calls] == [16 * kk, 16 * kk, 8 * kk]          # one call per user block, the short last one included
    assert all(type(x) is int for c in m.calls for x in c[0][:3] + c[1][:3])
    assert [u for c in m.calls for u in c[0]] == [int(r[0]) for r in rows]
    assert [i for c in m.calls for i in c[1]] == [int(r[1]) for r in rows]
