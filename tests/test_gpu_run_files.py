"""A VBPR run with every list flag on the MI355X: the results directory holds exactly the files of ranking.RUN_FILES, last epoch and
best epoch, and none of their bytes depends on the size of the evaluator's user blocks."""
import os

import pytest

from fashionvisualexpl_recommend_amd import evaluator, ranking
from test_gpu_new_items import _cli_dataset

pytestmark = pytest.mark.gpu

# the 14 names of a run with every flag, spelled out (not derived from the table under test)
PREFIXES = ("recs-", "expl-", "new-recs-", "new-expl-", "new-user-recs-", "sim-", "new-sim-", "div-recs-", "div-ild-",
            "div-new-user-recs-", "div-new-user-ild-", "because-", "because-new-recs-", "because-new-user-recs-")


def test_cli_writes_every_file_and_no_byte_depends_on_the_user_block(tmp_path, monkeypatch):
    from fashionvisualexpl_recommend_amd import train_rec
    paths, _, _ = _cli_dataset(tmp_path, "vbpr")                       # 30 users, 60 items
    rows = [("new shopper", 3), ("b", 7), ("new shopper", 9), ("c 3", 5), ("c 3", 6), ("new shopper", 40), ("c 3", 5)]
    (tmp_path / "new.tsv").write_text("".join("%s\t%d\n" % r for r in rows))
    # --batch_size 1: a step adds at most one term to a gradient row, so runs of the same seed agree bit for bit
    common = ["--rec", "vbpr", "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--reg", "0.01", "--top_k", "10", "--lr", "0.01", "--optimizer", "sgd", "--dtype", "bf16",
              "--feat_explain", "3", "--new_items"] + paths + \
             ["--new_users", str(tmp_path / "new.tsv"), "--fold_steps", "9", "--fold_negatives", "3", "--similar_items", "5",
              "--diversify", "0.5", "--diversify_pool", "25", "--because", "3"]
    res = [str(tmp_path / ("res%d" % q)) for q in range(2)]
    train_rec.train(common + ["--results_root", res[0]])
    m = train_rec._last_model
    assert m.evaluator.user_block >= 30                                # one block holds every user
    params = m.directory_parameters
    m.engine.close()
    init = evaluator.Evaluator.__init__

    def blocks_of_7(self, *args, **kwargs):                            # four full blocks and one of two users
        init(self, *args, **kwargs)
        self.user_block = 7
    monkeypatch.setattr(evaluator.Evaluator, "__init__", blocks_of_7)
    train_rec.train(common + ["--results_root", res[1]])
    assert train_rec._last_model.evaluator.user_block == 7
    train_rec._last_model.engine.close()
    rdir = [os.path.join(r, "rec_results", "toy", "vbpr") for r in res]
    files = sorted(os.listdir(rdir[0]))
    best = [f for f in files if f.startswith("best-recs-")]
    assert len(best) == 1 and best[0].endswith("-%s.tsv" % params)
    tails = {"": "2-%s.tsv" % params, "best-": best[0][len("best-recs-"):]}
    want = sorted([b + p + t for b, t in tails.items() for p in PREFIXES] + ["results-metrics-%s.pkl" % params])
    assert len(want) == 29 and files == want
    assert sorted(b + k + "-" for k in ranking.RUN_FILES for b in tails) == sorted(b + p for p in PREFIXES for b in tails)
    assert sorted(os.listdir(rdir[1])) == files
    for f in files:
        if f.endswith(".tsv"):
            one, two = (open(os.path.join(d, f), "rb").read() for d in rdir)
            assert one and one == two, f
