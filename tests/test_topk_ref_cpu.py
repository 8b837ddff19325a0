"""The row classifier and the row generator of the top-K edge tests (tests/topk_ref.py), pinned without a GPU: on every
DETERMINED row the classifier's unique answer is what the reference's own expression, row.argsort()[-K:][::-1]
(Evaluator.py:234), returns; the EITHER class stays too small to hide a failure; every family produces the rows it is named
after."""
from collections import Counter

import numpy as np
import pytest

import topk_ref as tr


def _classes(I, K):
    sc, train, fams = tr.gen_rows(I, K)
    m = tr.mask(sc, train)
    return m, train, fams, [tr.classify(m[r], K, tr.n_unmasked(I, train[r])) for r in range(len(fams))]


@pytest.mark.parametrize("I,K", tr.SHAPES)
def test_determined_rows_have_the_reference_answer(I, K):
    m, train, fams, cls = _classes(I, K)
    n = 0
    for r, c in enumerate(cls):
        if c != tr.DETERMINED:
            continue
        n += 1
        assert np.array_equal(tr.unique_topk(m[r], K), m[r].argsort()[-K:][::-1]), (fams[r], r)
    assert (n == 0) == (K > I)


def test_either_class_is_small_and_never_in_the_zero_denormal_inf_families():
    total, either = 0, 0
    for I, K in tr.SHAPES:
        _, _, fams, cls = _classes(I, K)
        total += len(cls)
        either += sum(c == tr.EITHER for c in cls)
        for f, c in zip(fams, cls):
            assert not (c == tr.EITHER and f in tr.NEVER_EITHER), (I, K, f)
    assert either <= 0.05 * total, (either, total)


@pytest.mark.parametrize("I,K", tr.SHAPES)
def test_families_produce_the_rows_they_are_named_after(I, K):
    m, train, fams, cls = _classes(I, K)
    by = {}
    for r, (f, c) in enumerate(zip(fams, cls)):
        by.setdefault(f, Counter())[c] += 1
    assert sum(n for _, n in tr.FAMILIES) == len(fams) and 96 <= len(fams) <= 110
    if K > I:
        assert set(cls) == {tr.MUST_FLAG}
        return
    for f in ("distinct", "denormal", "inf_one", "neg_inf", "zeros_below", "exact_k", "dup_train"):
        assert set(by[f]) == {tr.DETERMINED}, (f, by[f])
    for f in ("zeros_inside_pm", "zeros_inside_mp", "zeros_straddle_pm", "zeros_straddle_mp", "inf_two"):
        assert set(by[f]) == {tr.MUST_FLAG}, (f, by[f])
    assert set(by["k_minus_1"]) == {tr.EITHER}
    assert by["five_levels"][tr.MUST_FLAG] >= 6 or K == 1
    # the structure itself, on the masked rows
    for r, f in enumerate(fams):
        row, v = m[r], np.sort(m[r])[::-1]
        if f.startswith("zeros_"):
            z = np.nonzero(row == 0)[0]
            assert z.size == 2 and np.signbit(row[z]).sum() == 1
            rank = int((row > 0).sum())                       # the pair holds ranks rank, rank + 1
            inside, straddle = rank + 1 <= K - 1, rank == K - 1
            if f == "zeros_below":
                assert rank >= K
            elif K == 1:
                assert straddle                               # no room for a pair inside a list of one
            else:
                assert inside if f.startswith("zeros_inside") else straddle
            if f.endswith("_pm") or f.endswith("_mp"):
                plus = z[~np.signbit(row[z])][0]
                assert (plus == z.min()) == f.endswith("_pm")
        elif f == "denormal":
            fin = row[np.isfinite(row)]
            assert np.all(np.abs(fin) < 2.0 ** -126) and np.all(fin != 0) and np.unique(fin).size == fin.size
        elif f == "inf_one":
            assert (row == np.inf).sum() == 1
        elif f == "inf_two":
            assert (row == np.inf).sum() == 2
        elif f == "neg_inf":
            assert (row == -np.inf).sum() == len(set(train[r])) + 1
        elif f == "exact_k":
            assert tr.n_unmasked(I, train[r]) == K
        elif f == "k_minus_1":
            assert tr.n_unmasked(I, train[r]) == K - 1
        elif f == "dup_train":
            assert len(train[r]) > len(set(train[r]))
    both = {np.signbit(m[r][np.nonzero(m[r] == 0)[0].min()]) for r, f in enumerate(fams) if f == "zeros_below"}
    assert both == {True, False}                              # the pair below the boundary comes in both index orders


def test_classifier_on_hand_made_rows():
    inf = np.inf
    f = lambda *a: np.array(a, np.float32)
    assert tr.classify(f(3, 2, 1, 0), 2, 4) == tr.DETERMINED
    assert tr.classify(f(3, 0.0, -0.0, -1), 2, 4) == tr.MUST_FLAG          # +-0 straddle the boundary
    assert tr.classify(f(0.0, -0.0, -1, -2), 2, 4) == tr.MUST_FLAG         # +-0 inside the list
    assert tr.classify(f(3, 2, 0.0, -0.0), 2, 4) == tr.DETERMINED          # +-0 below it
    assert tr.classify(f(3, 2, 1), 4, 3) == tr.MUST_FLAG                   # K > I
    assert tr.classify(f(3, 2, -inf, -inf), 3, 2) == tr.EITHER             # fewer than K unmasked
    assert tr.classify(f(3, 2, -inf, -inf), 2, 2) == tr.DETERMINED         # exactly K unmasked
    assert tr.classify(f(inf, inf, 1, 0), 1, 4) == tr.MUST_FLAG
    assert tr.classify(f(3, 2, -inf, -5), 3, 4) == tr.DETERMINED           # a natural -inf below the list
    assert tr.classify(f(3, 2, -inf, -inf), 3, 3) == tr.EITHER             # a natural -inf AT the boundary, tied with a masked one
    assert tr.unique_topk(f(1, -0.0, 0.0, 5), 3).tolist() == [3, 0, 1]


def _emulated_failures(I, K, float_equality):
    sc, train, fams = tr.gen_rows(I, K)
    m = tr.mask(sc, train)
    out = [tr.emulate_topk(m[r], K, float_equality) for r in range(len(fams))]
    idx, val, flag = (np.stack([o[j] for o in out]) for j in range(3))
    return tr.check_launch(sc, train, fams, K, idx, val, flag, m)


@pytest.mark.parametrize("I,K", tr.SHAPES)
def test_checker_accepts_float_equality_and_rejects_bit_image_order(I, K):
    """The checks of the GPU test, run on a numpy selection by integer keys: clean when -0.0 shares the key of +0.0; with the
    bare bit image every failure is a row of a +-0.0 family inside or across the list, and there are such failures."""
    assert _emulated_failures(I, K, True) == []
    bad = _emulated_failures(I, K, False)
    assert all(f.startswith("zeros_inside") or f.startswith("zeros_straddle") for _, f, _, _ in bad), bad[:3]
    assert (len(bad) == 32) == (K <= I), len(bad)
