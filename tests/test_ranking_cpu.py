"""fashionvisualexpl_recommend_amd.ranking without a GPU or the library: the top-K entry is a stub built from the classifier
of tests/topk_ref.py.  It masks the lists into the (CPU) score tensor as the kernel does, answers DETERMINED rows with the unique
list, unflagged, and every other row with flag 1 and a POISONED list (idx -1, val nan): a flagged row's kernel output must not
be read.  Rows: gen_rows(70, 5) (most rows determined, every tie family among the rest) and gen_rows(70, 257) (K > I: every
row flagged, lists of 70).  The text is compared with the loops the writers held before they were folded into write_ranked,
restated here."""
import io

import numpy as np
import pytest
import torch

import topk_ref as tr
from fashionvisualexpl_recommend_amd import ranking

CASES = [(70, 5), (70, 257)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stub_topk(train, calls=None):
    def topk(scores, k):
        s = scores.numpy()                                    # (shares the tensor's memory: the mask lands IN `scores`)
        n, I = s.shape
        for r, t in enumerate(train):
            s[r, t] = -np.inf
        idx, val, flag = np.full((n, k), -1, np.int32), np.full((n, k), np.nan, np.float32), np.ones(n, np.int32)
        for r in range(n):
            if tr.classify(s[r], k, tr.n_unmasked(I, train[r])) == tr.DETERMINED:
                idx[r] = tr.unique_topk(s[r], k)
                val[r], flag[r] = s[r][idx[r]], 0
        if calls is not None:
            calls.append(flag.copy())
        return torch.from_numpy(idx), torch.from_numpy(val), torch.from_numpy(flag)
    return topk


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "I%d-K%d" % c)
def case(request):
    I, K = request.param
    sc, train, _ = tr.gen_rows(I, K)
    side = torch.from_numpy(np.random.RandomState(3).rand(sc.shape[0], I, 3).astype(np.float32))
    flags = []
    dev = torch.from_numpy(sc.copy())
    ids, vals, side_rows = ranking.rank_rows(_stub_topk(train, flags), dev, K, side)
    host = sc.copy()
    want = ranking.rank_rows_host(host, train, K)
    return dict(I=I, K=K, sc=sc, train=train, side=side.numpy(), flag=flags[0], ids=ids, vals=vals, side_rows=side_rows,
                want=want, masked_dev=dev.numpy(), masked_host=host)


def test_numpy_topk_is_the_references_expression():
    row = np.array([0.5, -0.0, 0.0, np.inf, -np.inf, 0.5, 3.0], np.float32)
    for k in (1, 3, 7, 12):
        assert np.array_equal(ranking.numpy_topk(row, k), row.argsort()[-k:][::-1])
    assert ranking.rows_per_block(4096, 300) == 4096 and ranking.rows_per_block(4096, 1 << 20) == 128
    assert ranking.rows_per_block(4096, 1 << 28) == 1 and ranking.rows_per_block(16, 0) == 16


def test_rank_rows_equals_rank_rows_host(case):
    K, I = case["K"], case["I"]
    kk = min(K, I)
    flagged = int(case["flag"].sum())
    assert flagged == len(case["flag"]) if K > I else 0 < flagged < len(case["flag"])      # both kinds of row are present
    ids, vals = case["ids"], case["vals"]
    wid, wval = case["want"]
    assert ids.shape == wid.shape == vals.shape == wval.shape == (len(case["train"]), kk)
    assert vals.dtype == np.float32 and wval.dtype == np.float32 and np.issubdtype(ids.dtype, np.integer)
    assert np.array_equal(ids, wid)
    assert np.array_equal(_bits(vals), _bits(wval))           # -0.0 and inf included
    assert np.array_equal(_bits(case["masked_dev"]), _bits(tr.mask(case["sc"], case["train"])))
    assert np.array_equal(_bits(case["masked_host"]), _bits(case["masked_dev"]))
    if K <= I:
        assert (_bits(vals) == 0x80000000).any() and np.isinf(vals).any()


def test_rank_rows_without_side_returns_none(case):
    ids, vals, none = ranking.rank_rows(_stub_topk(case["train"]), torch.from_numpy(case["sc"].copy()), case["K"])
    assert none is None and np.array_equal(ids, case["ids"]) and np.array_equal(_bits(vals), _bits(case["vals"]))


def test_side_rows_are_gathered_at_the_final_ids(case):
    side, ids, got = case["side"], case["ids"], case["side_rows"]
    assert got.shape == ids.shape + (3,) and got.dtype == np.float32
    for r in range(ids.shape[0]):                             # flagged rows: at numpy's ids, not at the kernel's
        assert np.array_equal(got[r], side[r, ids[r]]), (r, int(case["flag"][r]))


def test_rank_rows_host_without_masks():
    sc, _, _ = tr.gen_rows(70, 5)
    ids, vals = ranking.rank_rows_host(sc.copy(), None, 5)
    for r in range(sc.shape[0]):
        want = sc[r].argsort()[-5:][::-1]
        assert np.array_equal(ids[r], want) and np.array_equal(_bits(vals[r]), _bits(sc[r][want]))


# ---- the text: the loops of Evaluator._store_recommendation_device / _store_attention_rows before write_ranked, restated ------
def _parent_rows(labels, ids, vals, side=None):
    out, written = io.StringIO(), ([], [])
    for r, u in enumerate(labels):
        top_k_id, top_k_score = ids[r], vals[r]
        for i, value in enumerate(top_k_id):
            if side is None:
                out.write(str(u) + '\t' + str(value) + '\t' + str(top_k_score[i]) + '\n')
            else:
                a = side[r]
                out.write(str(u) + '\t' + str(value) + '\t' + str(top_k_score[i]) + '\t' + str(a[i, 0]) + '\t' +
                          str(a[i, 1]) + '\t' + str(a[i, 2]) + '\n')
        written[0].extend([u] * len(top_k_id))
        written[1].extend(int(v) for v in top_k_id)
    return out.getvalue(), written


@pytest.mark.parametrize("with_side", [False, True])
@pytest.mark.parametrize("labels", ["users", "names"])
def test_write_ranked_bytes_and_hook_arguments(case, labels, with_side):
    n = case["ids"].shape[0]
    lab = list(range(16, 16 + n)) if labels == "users" else ["new shopper %d" % r for r in range(n)]
    side = case["side_rows"] if with_side else None
    want_text, want_hook = _parent_rows(lab, case["ids"], case["vals"], side)
    out = io.StringIO()
    users, items = ranking.write_ranked(out, lab, case["ids"], case["vals"], side)
    assert out.getvalue().encode() == want_text.encode()
    assert (list(users), list(items)) == (want_hook[0], want_hook[1]) and all(type(i) is int for i in items)
    rows = want_text.splitlines()
    assert len(rows) == n * case["ids"].shape[1] and all(len(l.split('\t')) == (6 if with_side else 3) for l in rows)
    if case["K"] <= case["I"]:
        assert any(l.split('\t')[2] == "-0.0" for l in rows) and any(l.split('\t')[2] == "inf" for l in rows)
    # the kernel's int32 ids and numpy's int64 ids print alike; a float64 score would not print like the float32 one
    out32 = io.StringIO()
    ranking.write_ranked(out32, lab, case["ids"].astype(np.int32), case["vals"], side)
    assert out32.getvalue() == want_text


# ---- lists_to_csr: Evaluator._device_csr as it stood, restated -----------------------------------------------------------------
def _old_device_csr(lists, dedup=False):
    if dedup:
        lists = [list(dict.fromkeys(l)) for l in lists]
    indptr = np.zeros(len(lists) + 1, dtype=np.int64)
    for u, l in enumerate(lists):
        indptr[u + 1] = indptr[u] + len(l)
    items = np.fromiter((i for l in lists for i in l), dtype=np.int32, count=int(indptr[-1]))
    if items.size == 0:
        items = np.zeros(1, np.int32)
    return indptr, items


def test_lists_to_csr():
    ragged = [[5, 3, 5, 9], [], [2], [7, 7, 7], [], [0, 299, 1]]
    for dedup in (False, True):
        ptr, items = ranking.lists_to_csr(ragged, "cpu", dedup=dedup)
        wptr, witems = _old_device_csr(ragged, dedup)
        assert ptr.dtype == torch.int64 and items.dtype == torch.int32
        assert np.array_equal(ptr.numpy(), wptr) and np.array_equal(items.numpy(), witems)
    ptr, items = ranking.lists_to_csr(ragged, "cpu", dedup=True)
    assert items.tolist() == [5, 3, 9, 2, 7, 0, 299, 1] and ptr.tolist() == [0, 3, 3, 4, 5, 5, 8]      # first occurrences
    assert ranking.lists_to_csr([np.array([4, 1], np.int64), (2,)], "cpu")[1].tolist() == [4, 1, 2]
    for empty in ([[], [], []], []):
        ptr, items = ranking.lists_to_csr(empty, "cpu")
        assert ptr.tolist() == [0] * (len(empty) + 1) and items.tolist() == [0] and items.dtype == torch.int32


def test_ranking_does_not_load_the_library():
    import ast
    tree = ast.parse(open(ranking.__file__).read())
    mods = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    mods += [("." * n.level) + (n.module or "") for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert sorted(mods) == ["numpy", "torch"]                 # plain numpy + torch: nothing of the package, so no _ffi
