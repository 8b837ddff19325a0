"""Category shelves and quota lists on the CPU: the binding and the header name the entry, ranking.class_csr / rank_class_rows /
shelf_order / cap_rows / the two writers agree with the numpy restatement of tests/shelves_ref.py through a stub top-K (no
library call), SHELF_FILES names its files next to the three older tables, and the CLI rejects what it must.  No GPU."""
import io
import os
import re

import numpy as np
import pytest
import torch

import shelves_ref as sr
from fashionvisualexpl_recommend_amd import _ffi, ranking, train_rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_bound_and_declared():
    header = open(os.path.join(ROOT, "include", "bprx.h")).read()
    assert "bprx_topk_classes" in _ffi.EXPORTS and re.search(r"BPRX_API int bprx_topk_classes\(", header)
    assert _ffi.ABI_VERSION == 6 and re.search(r"#define BPRX_ABI_VERSION 6\b", header)
    src = open(os.path.join(ROOT, "fashionvisualexpl_recommend_amd", "_ffi.py")).read()
    assert re.search(r'"bprx_topk_classes": \(C\.c_int, \[vp, i64, i32, vp, i64, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp\]\)', src)


def test_class_csr_ragged_empty_and_classless():
    ptr, items, C = ranking.class_csr(np.array([2, -1, 0, 2, 0, 5, 2]), 7, "cpu")
    assert C == 6 and ptr.dtype == torch.int64 and items.dtype == torch.int32
    assert ptr.tolist() == [0, 2, 2, 5, 5, 5, 6]              # classes 1, 3 and 4 are empty, item 1 is on no list
    assert items.tolist() == [2, 4, 0, 3, 6, 5]               # ascending inside a class
    ptr, items, C = ranking.class_csr(np.full(4, -1), 4, "cpu")
    assert C == 1 and ptr.tolist() == [0, 0] and items.numel() == 1       # never an empty tensor
    for bad in (np.zeros(3, np.int64), np.zeros(4, np.float32), np.array([0, -2, 0, 0])):
        with pytest.raises(ValueError, match="class_csr"):
            ranking.class_csr(bad, 4, "cpu")


def _case(seed=3, n=9, width=41, C=5, ties=True):
    rs = np.random.RandomState(seed)
    sc = rs.standard_normal((n, width)).astype(np.float32)
    if ties:
        sc = np.round(sc * 2) / 2                             # many equal scores, both zeros
        sc[0, :7] = [0.0, -0.0, 0.0, -0.0, 1.5, 1.5, 1.5]
    item_class = rs.randint(-1, C, width)
    item_class[:7] = [0, 0, 1, 1, 2, 0, 2]
    lists = [rs.choice(width + 3, rs.randint(0, 6), replace=False).tolist() for _ in range(n)]
    return sc, item_class, lists


def _stub(lists, classes):
    """A top-K entry as rank_class_rows calls it: masks IN the block and returns the reference's lists as tensors."""
    def topk_classes(scores, k):
        m = sr.mask(scores.numpy(), lists)
        scores.copy_(torch.from_numpy(m))
        ids, vals, cnt = sr.class_lists(m, classes, k)
        return torch.from_numpy(ids.astype(np.int32)), torch.from_numpy(vals), torch.from_numpy(cnt.astype(np.int32))
    return topk_classes


@pytest.mark.parametrize("k", [1, 3, 60])
def test_rank_class_rows_order_and_cap_against_the_reference(k):
    sc, item_class, lists = _case()
    classes = sr.classes_of(item_class, 5)
    block = torch.from_numpy(sc.copy())
    ids, vals, cnt = ranking.rank_class_rows(_stub(lists, classes), block, k)
    kk = min(k, sc.shape[1])
    m = sr.mask(sc, lists)
    assert np.array_equal(sr.bits(block.numpy()), sr.bits(m))                  # masked in the caller's block
    wi, wv, wc = sr.class_lists(m, classes, kk)
    assert ids.dtype == np.int64 and cnt.dtype == np.int64 and ids.shape == (9, 5, kk)
    assert np.array_equal(ids, wi) and np.array_equal(sr.bits(vals), sr.bits(wv)) and np.array_equal(cnt, wc)
    got, want = ranking.shelf_order(vals, cnt), sr.shelf_order(wv, wc)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == 9
    for cap in (1, 2, kk, kk + 5):
        for top in (1, 4, 17, 300):
            K = min(cap, top)
            li, lv, lc = ranking.rank_class_rows(_stub(lists, classes), torch.from_numpy(sc.copy()), K)
            gi, gv, gc = ranking.cap_rows(li, lv, lc, top, cap)
            ri, rv, rc = sr.cap_lists(m, classes, top, cap)
            assert np.array_equal(gi, ri) and np.array_equal(sr.bits(gv), sr.bits(rv)) and np.array_equal(gc, rc), (cap, top)
            for r in range(9):                                                 # the cap holds
                assert all(int((gc[r] == c).sum()) <= cap for c in range(5))


def test_shelf_order_ties_zeros_and_empty_classes():
    vals = np.zeros((2, 4, 2), np.float32)
    vals[0, :, 0] = [1.0, 2.0, 1.0, 9.0]
    vals[1, :, 0] = [-0.0, 0.0, -1.0, 0.0]
    cnt = np.array([[1, 2, 1, 0], [1, 1, 1, 1]])
    got = ranking.shelf_order(vals, cnt)
    assert got[0].tolist() == [1, 0, 2]                      # class 3 is empty; equal scores by class id
    assert got[1].tolist() == [0, 1, 3, 2]                   # -0.0 == +0.0


def test_cap_at_least_k_is_the_plain_topk_on_a_tie_free_row():
    sc, item_class, lists = _case(seed=8, ties=False)
    item_class = np.abs(item_class)                           # every item has a class
    assert all(np.unique(r).size == r.size for r in sc)
    classes = sr.classes_of(item_class, 5)
    m = sr.mask(sc, lists)
    for k in (1, 6, 41):
        li, lv, lc = ranking.rank_class_rows(_stub(lists, classes), torch.from_numpy(sc.copy()), k)
        gi, gv, _ = ranking.cap_rows(li, lv, lc, k, k + 2)
        for r in range(sc.shape[0]):
            want = ranking.numpy_topk(m[r], k)
            want = want[m[r][want] > -np.inf]
            assert gi[r, :want.size].tolist() == want.tolist() and (gi[r, want.size:] == -1).all()
            assert np.array_equal(sr.bits(gv[r, :want.size]), sr.bits(m[r][want]))


def test_writers_format_as_write_ranked():
    ids = np.array([[[3, 1], [7, -1], [4, 5]]], np.int64)
    vals = np.array([[[2.5, 1.0], [2.5, 0.0], [-0.0, -1e-9]]], np.float32)
    cnt = np.array([[2, 1, 2]])
    out = io.StringIO()
    ranking.write_shelves(out, ["ann"], ids, vals, cnt)
    f = lambda x: str(np.float32(x))
    assert out.getvalue() == "".join("ann\t%d\t%d\t%s\n" % row for row in
                                     ((0, 3, f(2.5)), (0, 1, f(1.0)), (1, 7, f(2.5)), (2, 4, f(-0.0)), (2, 5, f(-1e-9))))
    out = io.StringIO()
    ranking.write_shelves(out, [7], ids, vals, cnt, 2)
    assert [l.split("\t")[:2] for l in out.getvalue().splitlines()] == [["7", "0"], ["7", "0"], ["7", "1"]]
    out = io.StringIO()
    ranking.write_capped(out, ["ann", 5], np.array([[3, 7, -1], [-1, -1, -1]]), np.array([[2.5, 2.5, 0], [0, 0, 0]], np.float32),
                         np.array([[0, 1, -1], [-1, -1, -1]]))
    assert out.getvalue() == "ann\t3\t2.5\t0\nann\t7\t2.5\t1\n"


def test_block_cut_keeps_scores_and_outputs_below_2_27():
    assert ranking.class_rows_per_block(4096, 50000, 16, 20) == (1 << 27) // 50000
    assert ranking.class_rows_per_block(4096, 1000, 256, 1024) == ((1 << 27) - 1) // (256 * 1024)
    assert ranking.class_rows_per_block(4096, 10, 2, 3) == 4096
    assert ranking.class_rows_per_block(4096, 1 << 28, 1 << 20, 1024) == 1          # never below one row
    for ub, w, C, K in ((4096, 50000, 16, 20), (4096, 1000, 256, 1024), (7, 60, 5, 3)):
        n = ranking.class_rows_per_block(ub, w, C, K)
        assert n * C * K < 1 << 27 and n * w <= 1 << 27 and n <= ub


def test_shelf_files_naming_and_disjointness():
    assert set(ranking.SHELF_FILES) == {"shelf-recs", "cap-recs", "shelf-new-user-recs", "cap-new-user-recs"}
    for other in (ranking.RUN_FILES, ranking.ITEM_FILES, ranking.WARM_FILES):
        assert not set(ranking.SHELF_FILES) & set(other)
    assert len(ranking.RUN_FILES) == 14 and set(ranking.ITEM_FILES) == {"audience", "new-audience"}
    assert set(ranking.WARM_FILES) == {"warm-recs", "warm-audience"}
    assert ranking.shelf_file("/r/recs-3-batch_8-K_4.tsv", "shelf-recs") == "/r/shelf-recs-3-batch_8-K_4.tsv"
    assert ranking.shelf_file("/r/best-recs-2-x.tsv", "cap-new-user-recs") == "/r/best-cap-new-user-recs-2-x.tsv"
    assert ranking.shelf_file("recs-1-x.tsv", "cap-recs") == "cap-recs-1-x.tsv"
    with pytest.raises(ValueError, match="recs"):
        ranking.shelf_file("/r/sim-3-x.tsv", "shelf-recs")
    with pytest.raises(ValueError, match="shelf_file"):
        ranking.shelf_file("/r/recs-3-x.tsv", "recs")


def test_category_lists_are_device_only_and_not_for_models_without_the_plain_score_block():
    from argparse import Namespace
    from fashionvisualexpl_recommend_amd.models import ACF, BPRMF, AttentiveFashion
    on_device = Namespace(diverse=True, evaluator=Namespace(force_host=False))
    BPRMF._class_args(on_device, 3, 2)
    with pytest.raises(ValueError, match="force_host"):
        BPRMF._class_args(Namespace(diverse=True, evaluator=Namespace(force_host=True)), 3, None)
    for k, cap in ((0, None), (1025, None), (3, 0)):
        with pytest.raises(ValueError, match="category lists"):
            BPRMF._class_args(on_device, k, cap)
    assert ACF.diverse is False and AttentiveFashion.diverse is False
    with pytest.raises(NotImplementedError, match="category lists"):
        BPRMF._class_args(Namespace(diverse=False, evaluator=Namespace(force_host=False)), 3, None)


def _tsv(tmp_path, text, name="classes.tsv"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_read_item_classes(tmp_path):
    good = _tsv(tmp_path, "2\t1\n0\t0\n\n1\t4\n")
    assert train_rec.read_item_classes(good).tolist() == [0, 4, 1]
    assert train_rec.read_item_classes(good, 3).tolist() == [0, 4, 1]
    with pytest.raises(ValueError, match=r"classes.tsv: the item 3 has no class"):
        train_rec.read_item_classes(good, 4)
    with pytest.raises(ValueError, match=r"classes.tsv:1: the item 2 is outside the catalogue"):
        train_rec.read_item_classes(good, 2)
    for text, line in (("0\t1\n0\t2\n", 2), ("0\t1\n1\n", 2), ("0\tx\n", 1), ("0\t-1\n", 1), ("-1\t0\n", 1), ("0\t1\t2\n", 1)):
        with pytest.raises(ValueError, match=r"bad.tsv:%d: " % line):
            train_rec.read_item_classes(_tsv(tmp_path, text, "bad.tsv"))


def test_dataset_item_classes_is_the_argmax_of_the_one_hot_vectors(tmp_path, monkeypatch):
    from fashionvisualexpl_recommend_amd import configs
    monkeypatch.setattr(configs, "_data_root", str(tmp_path))
    d = configs.class_features_path_dir("toy")
    os.makedirs(d)
    for i, c in enumerate([2, 0, 3]):
        v = np.zeros((1, 4), np.float32)
        v[0, c] = 1.0
        np.save(d + "%d.npy" % i, v)
    assert train_rec.dataset_item_classes("toy", 3).tolist() == [2, 0, 3]
    with pytest.raises(ValueError, match=r"3\.npy is missing"):
        train_rec.dataset_item_classes("toy", 4)
    args = train_rec.parse_args(["--rec", "vbpr", "--dataset", "toy", "--item_classes", "dataset", "--class_cap", "2"])
    train_rec.check_item_classes(args, 3)
    with pytest.raises(SystemExit):
        train_rec.check_item_classes(args, 4)


def test_parse_args_rejects(tmp_path, capsys):
    good = _tsv(tmp_path, "0\t0\n1\t1\n")
    for argv in (["--rec", "bprmf", "--shelves", "3"],                                         # no class table
                 ["--rec", "bprmf", "--class_cap", "2"],
                 ["--rec", "acf", "--item_classes", good, "--shelves", "3"],
                 ["--rec", "attentive_fashion", "--item_classes", good, "--class_cap", "2"],
                 ["--rec", "vbpr", "--item_classes", good, "--shelves", "-1"],
                 ["--rec", "vbpr", "--item_classes", good, "--shelves", "1025"],
                 ["--rec", "vbpr", "--item_classes", good, "--class_cap", "-1"],
                 ["--rec", "vbpr", "--item_classes", good, "--shelf_count", "2"],               # needs --shelves
                 ["--rec", "vbpr", "--item_classes", good, "--shelves", "3", "--shelf_count", "-1"],
                 ["--rec", "vbpr", "--item_classes", str(tmp_path / "missing.tsv"), "--shelves", "3"],
                 ["--rec", "vbpr", "--item_classes", _tsv(tmp_path, "0\t0\n0\t1\n", "twice.tsv"), "--shelves", "3"],
                 ["--rec", "vbpr", "--item_classes", _tsv(tmp_path, "0\tshoes\n", "word.tsv"), "--shelves", "3"]):
        with pytest.raises(SystemExit):
            train_rec.parse_args(argv)
        err = capsys.readouterr().err
        assert "shelves" in err or "class_cap" in err or "item_classes" in err or "shelf_count" in err, argv
    # a missing item and an item outside the catalogue: known once the data is loaded, rejected the same way
    args = train_rec.parse_args(["--rec", "bprmf", "--item_classes", good, "--shelves", "3", "--class_cap", "2"])
    assert (args.shelves, args.shelf_count, args.class_cap) == (3, 0, 2)
    train_rec.check_item_classes(args, 2)
    for n in (1, 3):
        with pytest.raises(SystemExit):
            train_rec.check_item_classes(args, n)
        assert "item_classes" in capsys.readouterr().err
    off = train_rec.parse_args(["--rec", "acf"])
    assert (off.shelves, off.shelf_count, off.class_cap, off.item_classes) == (0, 0, 0, None)
    assert train_rec.parse_args(["--rec", "grad_fashion", "--item_classes", "dataset", "--shelves", "1024"]).shelves == 1024
    for flag in ("--shelves", "--class_cap"):
        with pytest.raises(NotImplementedError, match="shelves"):
            train_rec.train(["--rec", "vbpr", "--item_classes", good, flag, "2", "--world_size", "2"])
