"""Style clusters without a GPU: the C ABI's two entries in the header and the binding, the flags of train_rec, the float64
restatement (tests/styles_ref.py) on planted data, the file names and writers, and the excusal check of the inputs that
tests/test_gpu_styles.py assigns."""
import io
import os
import re

import numpy as np
import pytest

import styles_ref as sr
from fashionvisualexpl_recommend_amd import _ffi, build, ranking, train_rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- header and binding ----------------------------------------------------------------------------------------------------
def _header_args(name):
    text = open(os.path.join(ROOT, "include", "bprx.h")).read()
    m = re.search(r"BPRX_API int %s\((.*?)\);" % name, text, re.S)
    assert m, name
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",") if a.strip()]


def test_header_and_binding_export_both_entries():
    text = open(os.path.join(ROOT, "include", "bprx.h")).read()
    assert re.search(r"#define BPRX_ABI_VERSION 6\b", text) and _ffi.ABI_VERSION == 6
    assert "bprx_styles.hip" in build.SOURCES
    src = open(_ffi.__file__).read()
    for name, nargs in (("bprx_style_assign", 13), ("bprx_style_update", 10)):
        assert len(_header_args(name)) == nargs
        assert name in _ffi.EXPORTS
        sig = re.search(r'"%s": \(C\.c_int, \[(.*?)\]\)' % name, src).group(1)
        assert len(sig.split(",")) == nargs
    assert re.search(r"#define BPRX_STYLES_MAX 1024\b", text)


# ---- parser ----------------------------------------------------------------------------------------------------------------
BASE = ["--dataset", "toy"]


def _ok(*flags):
    return train_rec.parse_args(BASE + list(flags))


def _rejected(capsys, *flags):
    with pytest.raises(SystemExit):
        train_rec.parse_args(BASE + list(flags))
    return capsys.readouterr().err


def test_parser_accepts_the_style_flags():
    a = _ok("--rec", "vbpr")
    assert (a.styles, a.style_iters, a.style_top) == (0, 20, 10)
    a = _ok("--rec", "vbpr", "--styles", "5", "--style_iters", "3", "--style_top", "1024")
    assert (a.styles, a.style_iters, a.style_top, a.similar_space) == (5, 3, 1024, "visual")
    assert _ok("--rec", "bprmf", "--styles", "2").similar_space == "latent"
    assert _ok("--rec", "grad_fashion", "--styles", "1024", "--similar_space", "both").similar_space == "both"
    a = _ok("--rec", "vbpr", "--styles", "4", "--item_classes", "styles", "--shelves", "3", "--class_cap", "2", "--new_items", "n.npy")
    assert a.item_classes == "styles"
    assert _ok("--rec", "vbpr", "--styles", "4", "--similar_space", "latent").similar_space == "latent"


@pytest.mark.parametrize("flags,words", [
    (("--rec", "vbpr", "--styles", "1"), "--styles"),
    (("--rec", "vbpr", "--styles", "1025"), "--styles"),
    (("--rec", "vbpr", "--styles", "-3"), "--styles"),
    (("--rec", "vbpr", "--styles", "4", "--style_iters", "0"), "--style_iters"),
    (("--rec", "vbpr", "--styles", "4", "--style_top", "0"), "--style_top"),
    (("--rec", "vbpr", "--styles", "4", "--style_top", "1025"), "--style_top"),
    (("--rec", "vbpr", "--style_top", "3"), "--styles"),
    (("--rec", "vbpr", "--style_iters", "3"), "--styles"),
    (("--rec", "acf", "--styles", "4"), "--styles"),
    (("--rec", "attentive_fashion", "--styles", "4"), "--styles"),
    (("--rec", "bprmf", "--styles", "4", "--similar_space", "visual"), "--similar_space"),
    (("--rec", "vbpr", "--styles", "4", "--dtype", "fp8"), "--similar_space"),
    (("--rec", "vbpr", "--item_classes", "styles", "--shelves", "3"), "--styles"),
])
def test_parser_rejects(capsys, flags, words):
    assert words in _rejected(capsys, *flags)


def test_new_items_need_the_visual_space_and_the_error_names_both_flags(capsys):
    err = _rejected(capsys, "--rec", "vbpr", "--styles", "4", "--similar_space", "latent", "--new_items", "n.npy")
    assert "--similar_space" in err and "--new_items" in err
    err = _rejected(capsys, "--rec", "vbpr", "--styles", "4", "--similar_space", "both", "--new_items", "n.npy")
    assert "--similar_space" in err and "--new_items" in err


# ---- the restatement on planted data -----------------------------------------------------------------------------------------
def test_reference_loop_recovers_a_planted_partition():
    z, label = sr.planted([1, 40, 64, 65, 130, 300], 16, 0.05, seed=3)
    rn = sr.rnorm(z)
    style, cos, cent, obj = sr.loop(z, rn, 6)
    assert sr.same_partition(style, label)
    assert len(obj) < 20 and (np.diff(obj) >= -sr.tol(16)).all()
    assert np.allclose(np.linalg.norm(cent, axis=1), 1.0, atol=1e-6) and (cos > 0.9).all()
    assert len(set(sr.seeds(z, rn, 6).tolist())) == 6 and set(label[sr.seeds(z, rn, 6)].tolist()) == set(range(6))


def test_reference_special_rows_and_degenerate_clusters():
    z = np.array([[1, 0], [0, 0], [-1, 0], [0, 2], [1, 0]], np.float32)
    rn = sr.rnorm(z)
    cent = np.array([[1, 0], [1, 0], [0, 0]], np.float32)
    style, best, second, gap = sr.assign(z, rn, cent)
    assert style.tolist() == [0, -1, 2, 0, 0] and best.tolist() == [1.0, 0.0, 0.0, 0.0, 1.0] and second[1] == 0.0
    assert sr.assign(z, rn, cent[:1])[2][0] == -np.inf
    prev = np.array([[0, 1], [0.6, 0.8], [1, 0]], np.float64)
    c, mass = sr.update(z, rn, [np.array([0, 2]), np.array([], np.int64), np.array([0, 3, 4])], prev)
    assert np.array_equal(c[:2], prev[:2]) and mass[:2].tolist() == [0.0, 0.0]
    assert np.allclose(c[2], np.array([2, 1]) / np.sqrt(5)) and np.isclose(mass[2], np.sqrt(5))
    with pytest.raises(ValueError):
        sr.seeds(z, rn, 5)


# ---- the inputs of the GPU tests: how many rows the reference would excuse -----------------------------------------------------
def _excused_share(z, cent):
    w = z.shape[1]
    gap = sr.assign(z, sr.rnorm(z), cent)[3]
    return sr.excused(gap, w).mean(), gap.min()


@pytest.mark.parametrize("I,w,S", sr.ASSIGN_CASES)
def test_assign_inputs_excuse_at_most_one_percent(I, w, S):
    share, smallest = _excused_share(*sr.assign_case(I, w, S))
    print("I=%d w=%d S=%d: excused %.4f, smallest gap %.3g, 2 tol %.3g" % (I, w, S, share, smallest, 2 * sr.tol(w)))
    assert share <= 0.01


def test_both_space_inputs_excuse_at_most_one_percent():
    _, _, _, z, cent = sr.both_case()
    share, smallest = _excused_share(z, cent)
    print("both: excused %.4f, smallest gap %.3g, 2 tol %.3g" % (share, smallest, 2 * sr.tol(z.shape[1])))
    assert share <= 0.01


# ---- file names and writers ---------------------------------------------------------------------------------------------------
def test_style_files_are_named_like_the_other_run_files():
    assert list(ranking.STYLE_FILES) == ["styles", "style-items", "user-styles", "new-styles"]
    assert ranking.style_file("/r/recs-3-p.tsv", "styles") == "/r/styles-3-p.tsv"
    assert ranking.style_file("/r/best-recs-3-p.tsv", "user-styles") == "/r/best-user-styles-3-p.tsv"
    for path, kind in (("/r/sim-3-p.tsv", "styles"), ("/r/recs-3-p.tsv", "shelf-recs")):
        with pytest.raises(ValueError):
            ranking.style_file(path, kind)


def test_writers():
    out = io.StringIO()
    ranking.write_styles(out, np.array([2, -1]), np.array([0.5, 0.0], np.float32))
    assert out.getvalue() == "0\t2\t0.5\n1\t-1\t0.0\n"
    out = io.StringIO()
    ranking.write_style_items(out, np.array([3, 0, 1]), np.array([[4, 1], [-1, -1], [2, -1]]),
                              np.array([[0.75, 0.5], [0, 0], [0.25, 0]], np.float32), np.array([2, 0, 1]))
    assert out.getvalue() == "0\t3\t0\t4\t0.75\n0\t3\t1\t1\t0.5\n2\t1\t0\t2\t0.25\n"
    rows = ranking.user_style_rows([[0, 1, 2, 3], [], [4, 4]], np.array([1, 0, 1, -1, 0]))
    assert [(r[0].tolist(), r[1].tolist(), r[2]) for r in rows] == [([1, 0], [2, 1], 4), ([], [], 0), ([0], [2], 2)]
    out = io.StringIO()
    ranking.write_user_styles(out, ["a", "b", "c"], rows)
    assert out.getvalue() == "a\t1\t2\t0.5\na\t0\t1\t0.25\nc\t0\t2\t1.0\n"


def test_class_csr_with_a_fixed_number_of_classes():
    ptr, items, C = ranking.class_csr(np.array([1, -1, 0, 1]), 4, "cpu", classes=4)
    assert C == 4 and ptr.tolist() == [0, 1, 3, 3, 3] and items.tolist() == [2, 0, 3]
    with pytest.raises(ValueError):
        ranking.class_csr(np.array([1, 5]), 2, "cpu", classes=4)
