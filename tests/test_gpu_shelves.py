"""bprx_topk_classes on the MI355X through Engine.topk_classes, compared EXACTLY with the numpy restatement of
tests/shelves_ref.py: ids equal, val bit-equal to the downloaded (masked) row at those ids, cnt equal, and the score buffer
afterwards the masked matrix bit for bit.  The kernel selects, it does not compute: no tolerance anywhere.

Shapes are the smallest at which each path of the kernel runs: class sizes around the wave (63 / 64 / 65), below and above the
wave's whole-class sort (<= 256) and above it (the workgroup's radix select, stopped where its bin fits the buffer, and run to its
end with the second select over item ids where more than 1 024 scores tie); K below and above every size; a row wider than
65 536; 1 501 classes in tiles of four; more rows than a launch takes workgroups along x."""
import gc
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import shelves_ref as sr
from fashionvisualexpl_recommend_amd import _ffi, evaluator, ranking, synth
from test_gpu_new_items import _cli_dataset

pytestmark = pytest.mark.gpu


def _bprmf(U=4, I=8):
    from fashionvisualexpl_recommend_amd.engine import Engine
    e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=4, optimizer="sgd", max_batch=8)
    return e.bind(Gu=np.zeros((U, 4), np.float32), Gi=np.zeros((I, 4), np.float32), Bi=np.zeros(I, np.float32))


@pytest.fixture(scope="module")
def eng():
    e = _bprmf()
    yield e
    e.sync_check()
    e.close()


def _csr(lists, dtype=np.int32):
    ptr = np.cumsum([0] + [len(l) for l in lists]).astype(np.int64)
    items = np.array([i for l in lists for i in l] or [0], dtype)
    return torch.as_tensor(ptr, device="cuda"), torch.as_tensor(items, device="cuda")


def _ccsr(classes):
    return _csr(classes) + (len(classes),)


def _run(e, sc, lists, classes, K, row0=0, all_lists=None):
    """One call: (ids, vals, cnt, the score buffer afterwards) as numpy.  all_lists: the mask CSR when it is longer than `lists`."""
    S = torch.as_tensor(np.ascontiguousarray(sc, dtype=np.float32), device="cuda").clone()
    mask = None if lists is None else _csr(lists if all_lists is None else all_lists)
    idx, val, cnt = e.topk_classes(S, mask, _ccsr(classes), K, row0)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and cnt.dtype == torch.int32
    assert tuple(idx.shape) == tuple(val.shape) == (sc.shape[0], len(classes), K) and tuple(cnt.shape) == (sc.shape[0], len(classes))
    return idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), cnt.cpu().numpy().astype(np.int64), S.cpu().numpy()


def _check(sc, lists, classes, K, got):
    ids, vals, cnt, after = got
    m = sr.mask(sc, lists)
    assert np.array_equal(sr.bits(after), sr.bits(m)), "the row is -inf at the masked ids and bit-unchanged elsewhere"
    wi, wv, wc = sr.class_lists(m, classes, K)
    assert np.array_equal(cnt, wc), np.argwhere(cnt != wc)[:5]
    assert np.array_equal(ids, wi), np.argwhere(ids != wi)[:5]
    assert np.array_equal(sr.bits(vals), sr.bits(wv)), np.argwhere(sr.bits(vals) != sr.bits(wv))[:5]
    on = ids >= 0
    rows = np.broadcast_to(np.arange(sc.shape[0])[:, None, None], ids.shape)
    assert np.array_equal(sr.bits(vals[on]), sr.bits(after[rows[on], ids[on]]))        # read from the row
    assert (vals[~on].view(np.uint32) == 0).all()                                      # +0.0 past cnt


def _split(width, sizes, seed):
    """Classes of the given sizes over a random permutation of [0, width): a list of ascending item arrays (0: an empty class)."""
    assert sum(sizes) <= width
    perm = np.random.RandomState(seed).permutation(width)
    cuts = np.cumsum([0] + list(sizes))
    return [np.sort(perm[cuts[c]:cuts[c + 1]]).astype(np.int64) for c in range(len(sizes))]


def _masks(n, width, most, seed):
    rs = np.random.RandomState(seed)
    return [rs.choice(width, rs.randint(0, most + 1), replace=False).tolist() for _ in range(n)]


# ---- 1. class-size edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5, 64, 300])
def test_class_size_edges(eng, K):
    n, width = 37, 1000
    classes = _split(width, [1, 2, 63, 0, 64, 65, 300, 505], seed=1)
    sc = np.random.RandomState(2).standard_normal((n, width)).astype(np.float32)
    assert all(np.unique(r).size == width for r in sc) and not (sc == 0).any()         # tie-free
    lists = _masks(n, width, 40, seed=3)
    _check(sc, lists, classes, K, _run(eng, sc, lists, classes, K))


# ---- 2. a row wider than 65 536 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [20, 1024])
def test_wide_row(eng, K):
    n, width = 3, 70000
    classes = _split(width, [69000, 999, 1], seed=4)
    sc = np.random.RandomState(5).standard_normal((n, width)).astype(np.float32)
    lists = _masks(n, width, 300, seed=6)
    _check(sc, lists, classes, K, _run(eng, sc, lists, classes, K))


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------
def _tie_rows(width, classes, K, seed):
    rs = np.random.RandomState(seed)
    rows = []
    for _ in range(4):                                       # multiples of 0.25 in [-2, 2], both zeros
        r = np.clip(np.round(rs.standard_normal(width) * 4) / 4, -2, 2).astype(np.float32)
        zero = np.flatnonzero(r == 0)
        r[zero[::2]] = -0.0
        assert (np.signbit(r) & (r == 0)).any() and (~np.signbit(r) & (r == 0)).any()
        rows.append(r)
    rows.append(-np.abs(rows[0]))                            # the two zeros on top of every class
    rows[-1][np.flatnonzero(rows[-1] == 0)[::2]] = 0.0
    rows.append(np.full(width, 0.75, np.float32))           # all equal
    for above in (0, 3):                                     # K - 1, K and K + 1 items at the K-th score, `above` items over them
        for t in (K - above - 1, K - above, K - above + 1):
            r = (-1.0 - rs.permutation(width) / width).astype(np.float32)       # distinct, all below
            for items in classes:
                if t < 1 or items.size < t + above:
                    continue
                pick = rs.permutation(items)
                r[pick[:above]] = 9.0 + np.arange(above, dtype=np.float32)
                r[pick[above:above + t]] = 5.0
            rows.append(r)
    r = (-1.0 - rs.permutation(width) / width).astype(np.float32)               # more equal scores than the kernel's buffer holds
    for items in classes:
        if items.size >= 1300:
            pick = rs.permutation(items)
            r[pick[:3]] = 9.0 + np.arange(3, dtype=np.float32)
            r[pick[3:1203]] = 5.0
    rows.append(r)
    return np.stack(rows)


@pytest.mark.parametrize("K", [1, 20, 300])
def test_ties_come_in_ascending_item_order(eng, K):
    width = 3000
    classes = _split(width, [1500, 700, 200, 600], seed=7)  # the workgroup's select three times, a wave's sort once
    sc = _tie_rows(width, classes, K, seed=8)
    lists = _masks(sc.shape[0], width, 25, seed=9)
    got = _run(eng, sc, lists, classes, K)
    _check(sc, lists, classes, K, got)
    ids, vals = got[0], got[1]
    zeros = vals[(ids >= 0) & (vals == 0)]
    if K >= 20:
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()                   # the sign of a zero is kept


# ---- 4. masks --------------------------------------------------------------------------------------------------------------
def test_masks_row0_null_and_ids_outside_the_row(eng):
    n, width, K = 6, 200, 9
    classes = _split(width, [50, 90, 20, 40], seed=10)
    sc = np.random.RandomState(11).standard_normal((n, width)).astype(np.float32)
    lists = _masks(n, width, 30, seed=12)
    lists[1] = sorted(set(lists[1]) | set(classes[2].tolist()))                        # the whole of class 2
    lists[2] = lists[2] + [width, width + 7, 100000, -1, -5] + lists[2][:2]            # ids outside the row; repeats
    got = _run(eng, sc, lists, classes, K)
    _check(sc, lists, classes, K, got)
    assert got[2][1, 2] == 0 and (got[0][1, 2] == -1).all() and got[2][0, 2] > 0
    # the same lists as rows 5 .. 10 of a longer CSR
    longer = _masks(5, width, 30, seed=13) + lists
    shifted = _run(eng, sc, lists, classes, K, row0=5, all_lists=longer)
    for a, b in zip(got, shifted):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    # list_ptr NULL: nothing is masked, the buffer keeps its bits
    plain = _run(eng, sc, None, classes, K)
    _check(sc, None, classes, K, plain)
    assert np.array_equal(sr.bits(plain[3]), sr.bits(sc))


# ---- 5. independence -------------------------------------------------------------------------------------------------------
def test_a_list_depends_on_its_row_and_its_class_only(eng):
    n, width, K = 8, 2500, 7
    sizes = [1200, 600, 130, 3, 500]
    classes = _split(width, sizes, seed=14)
    rs = np.random.RandomState(15)
    sc = (np.round(rs.standard_normal((n, width)) * 8) / 8).astype(np.float32)         # with ties
    lists = _masks(n, width, 30, seed=16)
    base = _run(eng, sc, lists, classes, K)
    _check(sc, lists, classes, K, base)
    same = lambda a, b: np.array_equal(a, b) if a.dtype != np.float32 else np.array_equal(sr.bits(a), sr.bits(b))
    perm = rs.permutation(n)                                                           # the rows in another order
    got = _run(eng, sc[perm], [lists[p] for p in perm], classes, K)
    assert all(same(g, b[perm]) for g, b in zip(got[:3], base[:3]))
    renum = rs.permutation(len(classes))                                               # class c is called renum[c]
    moved = [None] * len(classes)
    for c, to in enumerate(renum):
        moved[to] = classes[c]
    got = _run(eng, sc, lists, moved, K)
    assert all(same(g[:, renum], b) for g, b in zip(got[:3], base[:3]))
    for c in (0, 2):                                                                   # other classes' scores change
        other = sc.copy()
        out = np.setdiff1d(np.arange(width), classes[c])
        other[:, out] = rs.standard_normal((n, out.size)).astype(np.float32)
        got = _run(eng, other, lists, classes, K)
        assert all(same(g[:, c], b[:, c]) for g, b in zip(got[:3], base[:3]))


# ---- 6. many small classes -------------------------------------------------------------------------------------------------
def test_many_small_classes(eng):
    n, width, K = 5, 2000, 3
    perm = np.random.RandomState(17).permutation(width)
    classes = [np.array([i], np.int64) for i in perm[:1500]]
    classes.insert(701, np.sort(perm[1500:]).astype(np.int64))                         # the rest, inside a tile of singletons
    assert len(classes) == 1501
    sc = np.random.RandomState(18).standard_normal((n, width)).astype(np.float32)
    lists = _masks(n, width, 200, seed=19)
    _check(sc, lists, classes, K, _run(eng, sc, lists, classes, K))


# ---- 6b. more workgroups than a launch takes along x ------------------------------------------------------------------------
def test_more_rows_than_one_grid_row(eng):
    """Both launches fold their workgroup count into (x <= 2^22, y): 2^22 + 5 rows of four singleton classes, K = 1, so that the
    last rows sit in the grid's second row; row r masks item r % 4 where r % 3 == 0.  Checked whole, vectorised."""
    n, width = (1 << 22) + 5, 4
    sc = np.random.RandomState(29).standard_normal((n, width)).astype(np.float32)
    rows = np.arange(n)
    masked = rows % 3 == 0
    ptr = torch.as_tensor(np.concatenate([[0], np.cumsum(masked)]).astype(np.int64), device="cuda")
    items = torch.as_tensor((rows[masked] % 4).astype(np.int32), device="cuda")
    S = torch.as_tensor(sc, device="cuda").clone()
    idx, val, cnt = eng.topk_classes(S, (ptr, items), _ccsr([np.array([c]) for c in range(4)]), 1)
    want = sc.copy()
    want[rows[masked], rows[masked] % 4] = -np.inf
    on = want > -np.inf
    assert np.array_equal(sr.bits(S.cpu().numpy()), sr.bits(want))
    assert np.array_equal(cnt.cpu().numpy(), on.astype(np.int32))
    assert np.array_equal(idx.cpu().numpy()[:, :, 0], np.where(on, np.arange(4, dtype=np.int32)[None, :], -1))
    assert np.array_equal(sr.bits(val.cpu().numpy()[:, :, 0]), sr.bits(np.where(on, want, np.float32(0.0))))
    eng.sync_check()


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------
def test_arguments_errors_and_no_allocation(eng):
    lib = _ffi.lib()
    gc.collect()
    n, width, K = 4, 300, 5
    classes = _split(width, [100, 150, 50], seed=20)
    sc = np.random.RandomState(21).standard_normal((n, width)).astype(np.float32)
    lists = _masks(n, width, 10, seed=22)
    S = torch.as_tensor(sc, device="cuda").clone()
    mp, mi = _csr(lists)
    cp, ci, C = _ccsr(classes)
    idx = torch.empty((n, C, K), dtype=torch.int32, device="cuda")
    val = torch.empty((n, C, K), dtype=torch.float32, device="cuda")
    cnt = torch.empty((n, C), dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    live = lib.bprx_live_device_allocs()

    def call(nrows=n, w=width, s=S, row0=0, lp=mp, li=mi, cptr=cp, citems=ci, c=C, k=K, i=idx, v=val, ct=cnt):
        rc = lib.bprx_topk_classes(eng.h, nrows, w, p(s), row0, p(lp), p(li), p(cptr), p(citems), c, k, p(i), p(v), p(ct), None)
        assert lib.bprx_live_device_allocs() == live
        return rc

    bad = (dict(k=0), dict(k=1025), dict(k=-1), dict(c=0), dict(w=0), dict(nrows=-1), dict(row0=-1),
           dict(nrows=1 << 21, c=1024, k=1024), dict(nrows=2048, c=1024, k=1024), dict(nrows=1 << 31, c=1, k=1),
           dict(s=None), dict(cptr=None), dict(citems=None), dict(i=None), dict(v=None), dict(ct=None), dict(li=None))
    for kw in bad:
        assert call(**kw) == _ffi.E_INVALID, kw
        assert lib.bprx_last_error(eng.h)
    assert call(nrows=0) == 0
    assert call(nrows=0, s=None, lp=None, li=None, cptr=None, citems=None, i=None, v=None, ct=None) == 0
    assert lib.bprx_topk_classes(None, n, width, p(S), 0, p(mp), p(mi), p(cp), p(ci), C, K, p(idx), p(val), p(cnt), None) == _ffi.E_INVALID
    for k in (0, 1025):
        with pytest.raises(_ffi.BprxError) as err:
            eng.topk_classes(S, (mp, mi), (cp, ci, C), k)
        assert err.value.code == _ffi.E_INVALID
    # the handle is usable afterwards
    assert call() == 0
    eng.sync_check()
    _check(sc, lists, classes, K, (idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), cnt.cpu().numpy().astype(np.int64),
                                   S.cpu().numpy()))
    # class_items outside the row: skipped, the lists of the valid items are right, and the range error is reported once
    wrong = [np.concatenate([classes[0], [width, 10 ** 6]]), np.concatenate([[-3], classes[1]]), classes[2]]
    got = _run(eng, sc, lists, wrong, K)
    assert lib.bprx_live_device_allocs() == live
    with pytest.raises(_ffi.BprxError) as err:
        eng.sync_check()
    assert err.value.code == _ffi.E_RANGE
    eng.sync_check()
    _check(sc, lists, classes, K, got)


# ---- 8. leaves training alone ----------------------------------------------------------------------------------------------
def _params(opt):
    return Namespace(dataset="toy", validation=True, batch_size=64, epochs=1, batch_eval=128, embed_k=16, embed_d=12, lr=0.05,
                     reg=1e-3, top_k=10, verbose=-1, restore_epochs=1, rec="vbpr", best_metric="ndcg", optimizer=opt, init_seed=5,
                     dtype="bf16")


@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
def test_a_call_between_steps_leaves_the_run_bit_identical(opt):
    from fashionvisualexpl_recommend_amd.models import VBPR
    from test_gpu_feat_explain import _unique_batches
    U, I = 300, 600
    tr, va, te = synth.make_interactions(U, I, per_user=8, seed=23)
    data = Namespace(training_list=tr, validation_list=va, test_list=te, num_users=U, num_items=I, params=_params(opt))
    item_class = np.random.RandomState(24).randint(-1, 6, I)
    batches = _unique_batches(U, I, 64, 6, seed=25)
    end = []
    for with_call in (False, True):
        m = VBPR(data, _params(opt), features=synth.make_features(I, 128, seed=26))
        for s, b in enumerate(batches):
            if s == 3 and with_call:
                ids, vals, cnt = m.recommend_by_class(k=4, classes=item_class)
                assert ids.shape == (U, 6, 4) and cnt.max() == 4
                own = np.zeros((U, I), bool)
                for u in range(U):
                    own[u, tr[u]] = True
                on = ids >= 0
                assert not own[np.broadcast_to(np.arange(U)[:, None, None], ids.shape)[on], ids[on]].any()
                assert (item_class[ids[on]] == np.broadcast_to(np.arange(6)[None, :, None], ids.shape)[on]).all()
            m.engine.step(*b)
        m.engine.sync_check()
        end.append({n: v.cpu().numpy() for n, v in m.engine.t.items() if n != "F"})
        m.engine.close()
    for n in end[0]:
        a, b = (np.ascontiguousarray(x[n]) for x in end)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), n


# ---- 9. end to end ---------------------------------------------------------------------------------------------------------
def _rows(path):
    return [l.rstrip("\n").split("\t") for l in open(path)]


def test_cli_writes_shelves_and_capped_lists_next_to_unchanged_files(tmp_path, monkeypatch):
    from fashionvisualexpl_recommend_amd import train_rec
    _cli_dataset(tmp_path, "vbpr")                                     # 30 users, 60 items
    U, I, top_k = 30, 60, 10
    item_class = np.random.RandomState(27).randint(0, 5, I)
    item_class[:5] = np.arange(5)
    (tmp_path / "classes.tsv").write_text("".join("%d\t%d\n" % (i, item_class[i]) for i in np.random.RandomState(28).permutation(I)))
    new = [("new shopper", 3), ("b", 7), ("new shopper", 9), ("c 3", 5), ("c 3", 6), ("new shopper", 40), ("c 3", 5)]
    (tmp_path / "new.tsv").write_text("".join("%s\t%d\n" % r for r in new))
    # --batch_size 1: a step adds at most one term to a gradient row, so runs of the same seed agree bit for bit
    common = ["--rec", "vbpr", "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--reg", "0.01", "--top_k", str(top_k), "--lr", "0.01", "--optimizer", "sgd", "--dtype", "bf16",
              "--new_users", str(tmp_path / "new.tsv"), "--fold_steps", "9", "--fold_negatives", "3"]
    flags = ["--item_classes", str(tmp_path / "classes.tsv"), "--shelves", "3", "--shelf_count", "2", "--class_cap", "2"]
    res = [str(tmp_path / ("res%d" % q)) for q in range(4)]
    rdir = [os.path.join(r, "rec_results", "toy", "vbpr") for r in res]
    train_rec.train(common + flags + ["--results_root", res[0]])
    m = train_rec._last_model
    assert m.evaluator.user_block >= U
    params = m.directory_parameters
    train = [list(l) for l in m.data.training_list[:U]]
    scores = m.engine.score_block(0, U).cpu().numpy()                  # the final model: what recs-2-* was ranked from
    labels, histories = train_rec.read_new_users(str(tmp_path / "new.tsv"))
    fitted = m._fold_rows(histories, steps=9, negatives=3, seed=0)     # the fit _store_new_user_recs makes (no atomics: repeatable)
    new_scores = m._score_fold_rows(fitted, 0, len(labels))[0].cpu().numpy()
    m.engine.close()
    train_rec.train(common + ["--results_root", res[1]])
    train_rec._last_model.engine.close()
    with_flags, without = sorted(os.listdir(rdir[0])), sorted(os.listdir(rdir[1]))
    best = [f for f in without if f.startswith("best-recs-")]
    assert len(best) == 1
    tails = {"": "2-%s.tsv" % params, "best-": best[0][len("best-recs-"):]}
    extra = sorted(b + k + "-" + t for b, t in tails.items() for k in ("shelf-recs", "cap-recs", "shelf-new-user-recs", "cap-new-user-recs"))
    assert sorted(set(with_flags) - set(without)) == extra and set(without) <= set(with_flags)
    assert sorted(b + k + "-" + t for b, t in tails.items() for k in ranking.SHELF_FILES) == extra
    for f in without:                                                  # recs-*, best-recs-*, new-user-recs-*: not a byte moves
        if f.endswith(".tsv"):
            assert open(os.path.join(rdir[0], f), "rb").read() == open(os.path.join(rdir[1], f), "rb").read(), f
    assert {"recs-" + tails[""], "best-recs-" + tails["best-"], "new-user-recs-" + tails[""]} <= set(without)
    # shelf-recs-2-*: the reference's shelves of the final model's rows, as text
    classes = sr.classes_of(item_class, 5)
    masked = sr.mask(scores, train)
    ids, vals, cnt = sr.class_lists(masked, classes, 3)
    order = sr.shelf_order(vals, cnt)
    want = "".join("%d\t%d\t%d\t%s\n" % (u, c, ids[u, c, q], str(vals[u, c, q]))
                   for u in range(U) for c in order[u][:2] for q in range(cnt[u, c]))
    assert open(os.path.join(rdir[0], "shelf-recs-" + tails[""])).read() == want
    ci, cv, cc = sr.cap_lists(masked, classes, top_k, 2)
    want = "".join("%d\t%d\t%s\t%d\n" % (u, ci[u, q], str(cv[u, q]), cc[u, q]) for u in range(U) for q in range(top_k) if ci[u, q] >= 0)
    assert open(os.path.join(rdir[0], "cap-recs-" + tails[""])).read() == want
    # shelf-new-user-recs-2-* / cap-new-user-recs-2-*: the same restatement over the fitted rows' scores, the label's history masked
    nm = sr.mask(new_scores, histories)
    ids, vals, cnt = sr.class_lists(nm, classes, 3)
    order = sr.shelf_order(vals, cnt)
    want = "".join("%s\t%d\t%d\t%s\n" % (labels[r], c, ids[r, c, q], str(vals[r, c, q]))
                   for r in range(len(labels)) for c in order[r][:2] for q in range(cnt[r, c]))
    assert open(os.path.join(rdir[0], "shelf-new-user-recs-" + tails[""])).read() == want
    ci, cv, cc = sr.cap_lists(nm, classes, top_k, 2)
    want = "".join("%s\t%d\t%s\t%d\n" % (labels[r], ci[r, q], str(cv[r, q]), cc[r, q])
                   for r in range(len(labels)) for q in range(top_k) if ci[r, q] >= 0)
    assert open(os.path.join(rdir[0], "cap-new-user-recs-" + tails[""])).read() == want
    hist = {}
    for label, item in new:
        hist.setdefault(label, set()).add(item)
    for b, t in tails.items():
        for kind, own in (("shelf-recs", lambda u: train[int(u)]), ("shelf-new-user-recs", lambda u: hist[u])):
            rows = _rows(os.path.join(rdir[0], b + kind + "-" + t))
            assert rows and all(len(r) == 4 for r in rows)
            assert all(item_class[int(r[2])] == int(r[1]) and int(r[2]) not in own(r[0]) for r in rows)
            for u in dict.fromkeys(r[0] for r in rows):
                mine = [r for r in rows if r[0] == u]
                shelves = list(dict.fromkeys(r[1] for r in mine))
                assert 1 <= len(shelves) <= 2 and all(1 <= sum(r[1] == c for r in mine) <= 3 for c in shelves)
                for c in shelves:
                    s = [np.float32(r[3]) for r in mine if r[1] == c]
                    assert s == sorted(s, reverse=True)
                heads = [np.float32(next(r[3] for r in mine if r[1] == c)) for c in shelves]
                assert heads == sorted(heads, reverse=True)
            assert list(dict.fromkeys(r[0] for r in rows)) == ([str(u) for u in range(U)] if kind == "shelf-recs" else list(hist))
        for kind, own in (("cap-recs", lambda u: train[int(u)]), ("cap-new-user-recs", lambda u: hist[u])):
            rows = _rows(os.path.join(rdir[0], b + kind + "-" + t))
            assert rows and all(len(r) == 4 for r in rows)
            assert all(item_class[int(r[1])] == int(r[3]) and int(r[1]) not in own(r[0]) for r in rows)
            for u in dict.fromkeys(r[0] for r in rows):
                mine = [r for r in rows if r[0] == u]
                assert len(mine) == top_k and all(sum(r[3] == c for r in mine) <= 2 for c in "01234")
                s = [np.float32(r[2]) for r in mine]
                assert s == sorted(s, reverse=True) and len({r[1] for r in mine}) == top_k
    # --class_cap top_k caps nothing: the (u, i, score) of cap-recs-* are the rows of recs-*
    train_rec.train(common + ["--item_classes", str(tmp_path / "classes.tsv"), "--class_cap", str(top_k), "--results_root", res[2]])
    m = train_rec._last_model
    rows_of = sr.mask(m.engine.score_block(0, U).cpu().numpy(), train)
    m.engine.close()
    assert all(np.unique(r[r > -np.inf]).size == (r > -np.inf).sum() for r in rows_of)             # tie-free
    for b, t in tails.items():
        capped, recs = _rows(os.path.join(rdir[2], b + "cap-recs-" + t)), _rows(os.path.join(rdir[2], b + "recs-" + t))
        assert len(recs) == U * top_k and [r[:3] for r in capped] == recs
        assert open(os.path.join(rdir[2], b + "recs-" + t), "rb").read() == open(os.path.join(rdir[1], b + "recs-" + t), "rb").read()
    # user blocks of 7: the same bytes
    init = evaluator.Evaluator.__init__

    def blocks_of_7(self, *args, **kwargs):
        init(self, *args, **kwargs)
        self.user_block = 7
    monkeypatch.setattr(evaluator.Evaluator, "__init__", blocks_of_7)
    train_rec.train(common + flags + ["--results_root", res[3]])
    assert train_rec._last_model.evaluator.user_block == 7
    train_rec._last_model.engine.close()
    assert sorted(os.listdir(rdir[3])) == with_flags
    for f in with_flags:
        if f.endswith(".tsv"):
            assert open(os.path.join(rdir[0], f), "rb").read() == open(os.path.join(rdir[3], f), "rb").read(), f
