"""The naming table of a run's files (ranking.RUN_FILES / run_file, with div_paths and because_paths as its callers) and the two
block walks every ranking loop uses (ranking.blocks, ranking.wanted_blocks).  Plain Python: no GPU, no library."""
import os

import numpy as np
import pytest

from fashionvisualexpl_recommend_amd import ranking

# what a run with every flag writes next to recs-<e>-<params>.tsv, spelled out (not derived from the table under test)
NAMES = {"recs": "recs-", "expl": "expl-", "new-recs": "new-recs-", "new-expl": "new-expl-", "new-user-recs": "new-user-recs-",
         "sim": "sim-", "new-sim": "new-sim-", "div-recs": "div-recs-", "div-ild": "div-ild-",
         "div-new-user-recs": "div-new-user-recs-", "div-new-user-ild": "div-new-user-ild-", "because": "because-",
         "because-new-recs": "because-new-recs-", "because-new-user-recs": "because-new-user-recs-"}
TAIL = "2-batch_64-D_8-K_16-lr_0.001-reg_0.0.tsv"


@pytest.mark.parametrize("best", ["", "best-"])
def test_every_kind_maps_to_its_name(best):
    assert sorted(ranking.RUN_FILES) == sorted(NAMES) and len(NAMES) == 14
    for d in ("", os.path.join("res", "rec_results", "toy", "vbpr")):
        base = os.path.join(d, best + "recs-" + TAIL)
        for kind, prefix in NAMES.items():
            assert ranking.run_file(base, kind) == os.path.join(d, best + prefix + TAIL), kind
        # the two public callers agree with the table, for every list file they take
        at = lambda kind: ranking.run_file(base, kind)
        assert ranking.div_paths(base) == (at("div-recs"), at("div-ild"))
        assert ranking.div_paths(at("new-user-recs")) == (at("div-new-user-recs"), at("div-new-user-ild"))
        assert ranking.because_paths(base) == at("because")
        assert ranking.because_paths(at("new-recs")) == at("because-new-recs")
        assert ranking.because_paths(at("new-user-recs")) == at("because-new-user-recs")
    assert ranking.run_file(best + "recs-host.tsv", "expl") == best + "expl-host.tsv"      # (anything may follow the prefix)


def test_a_path_that_is_no_list_file_raises():
    d = os.path.join("res", "toy")
    for bad in ("results-metrics-x.pkl", "expl-" + TAIL, "sim-" + TAIL, "new-recs-" + TAIL, "new-user-recs-" + TAIL, "div-recs-" + TAIL,
                "best-expl-" + TAIL, "best-" + TAIL, "my-recs-" + TAIL, "recs" + TAIL, "bestrecs-" + TAIL, ""):
        for path in (bad, os.path.join(d, bad)):
            with pytest.raises(ValueError):
                ranking.run_file(path, "expl")
    with pytest.raises(ValueError):
        ranking.run_file(os.path.join("recs-dir", "x.tsv"), "expl")      # the file's name decides, not its directory's
    with pytest.raises(ValueError):
        ranking.run_file("recs-" + TAIL, "because-div-recs")             # no such kind
    for best in ("", "best-"):
        for bad in ("expl-", "sim-", "new-sim-", "div-recs-", "div-ild-", "div-new-user-recs-", "because-", "results-"):
            with pytest.raises(ValueError):
                ranking.because_paths(os.path.join(d, best + bad + TAIL))
        for bad in ("expl-", "sim-", "new-recs-", "div-recs-", "because-", "because-new-user-recs-", "results-"):
            with pytest.raises(ValueError):
                ranking.div_paths(os.path.join(d, best + bad + TAIL))


# ---- blocks ----------------------------------------------------------------------------------------------------------------------
def test_blocks():
    assert list(ranking.blocks(0, 4)) == []
    assert list(ranking.blocks(3, 4)) == [(0, 3)]                                        # smaller than one block
    assert list(ranking.blocks(12, 4)) == [(0, 4), (4, 8), (8, 12)]                      # an exact multiple
    assert list(ranking.blocks(30, 7)) == [(0, 7), (7, 14), (14, 21), (21, 28), (28, 30)]   # a last partial block
    assert list(ranking.blocks(1, 1)) == [(0, 1)]
    # the width cuts the block exactly as rows_per_block says: not at all, to 128 rows, to a single row
    assert list(ranking.blocks(10, 4, 300)) == list(ranking.blocks(10, 4))
    assert list(ranking.blocks(300, 4096, 1 << 20)) == [(0, 128), (128, 256), (256, 300)]
    assert list(ranking.blocks(3, 4096, 1 << 27)) == [(0, 1), (1, 2), (2, 3)]
    assert list(ranking.blocks(3, 4096, 1 << 30)) == [(0, 1), (1, 2), (2, 3)]
    assert list(ranking.blocks(5, 2, 0)) == [(0, 2), (2, 4), (4, 5)]
    for n, block, width in ((1000, 64, None), (1000, 4096, 1 << 19), (77, 7, 5)):        # a partition of [0, n), in order
        got = list(ranking.blocks(n, block, width))
        step = block if width is None else ranking.rows_per_block(block, width)
        assert got[0][0] == 0 and got[-1][1] == n and all(a[1] == b[0] for a, b in zip(got, got[1:]))
        assert all(b1 - b0 == step for b0, b1 in got[:-1]) and 0 < got[-1][1] - got[-1][0] <= step


def _wanted(want, n, block, width=None):
    want = np.asarray(want, dtype=np.int64)
    got = list(ranking.wanted_blocks(want, n, block, width))
    every = list(ranking.blocks(n, block, width))
    assert [(b0, b1) for b0, b1, _, _ in got] == [b for b in every if ((want >= b[0]) & (want < b[1])).any()]   # ascending, once
    seen = np.zeros(want.size, int)
    for b0, b1, rows, local in got:
        assert rows.size and (np.diff(rows) > 0).all()                                   # the caller's order
        assert np.array_equal(want[rows], local + b0) and (local >= 0).all() and (local < b1 - b0).all()
        seen[rows] += 1
    assert (seen == 1).all()                                                             # every wanted row, in exactly one block
    return [(b0, b1, rows.tolist(), local.tolist()) for b0, b1, rows, local in got]


def test_wanted_blocks():
    assert _wanted([], 40, 16) == []
    assert _wanted([33, 2, 2, 39], 40, 16) == [(0, 16, [1, 2], [2, 2]), (32, 40, [0, 3], [1, 7])]      # non-adjacent blocks, a repeat
    assert _wanted([39, 20, 17, 3], 40, 16) == [(0, 16, [3], [3]), (16, 32, [1, 2], [4, 1]), (32, 40, [0], [7])]     # descending ids
    assert _wanted([5, 5, 5], 6, 4) == [(4, 6, [0, 1, 2], [1, 1, 1])]
    assert _wanted(np.arange(30), 30, 7) == [(b0, b1, list(range(b0, b1)), list(range(b1 - b0))) for b0, b1 in ranking.blocks(30, 7)]
    assert _wanted([2, 0], 3, 4096, 1 << 27) == [(0, 1, [1], [0]), (2, 3, [0], [0])]     # a width that leaves one row per block
    rs = np.random.RandomState(5)
    for n, block, width in ((1000, 64, None), (500, 4096, 1 << 21), (9, 2, None)):
        _wanted(rs.randint(0, n, 50), n, block, width)
