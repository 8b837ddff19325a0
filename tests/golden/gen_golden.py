#!/usr/bin/env python3
"""One-off generator of the golden fixtures in tests/golden/ (run in the BUILD container only).

It executes the two pieces of the reference hot path that run without TensorFlow,
unmodified and read-only from the reference checkout's src/ directory (the first argument):
  * DataLoader.all_triple_batches   (src/dataset/dataset.py:83-114)  -> index-stream fixtures
  * Evaluator.eval / store_recommendation (src/recommender/Evaluator.py:149-239) -> metric fixtures
dataset.py line 3 does `import tensorflow as tf`; the sampled code never touches `tf`, so an EMPTY
module object is registered under that name to let the import statement succeed (SURVEY 8(c) recipe).
Nothing else of the reference is stubbed, and no reference source is copied: the outputs written here
are data (inputs + expected outputs) only.  The reference does not exist on the GPU box; tests read
only the files this script wrote.

    python tests/golden/gen_golden.py <reference>/src     # rewrites tests/golden/*.npz / *.json / *.tsv
"""
import hashlib
import json
import os
import random
import sys
import tempfile
import types
from argparse import Namespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_SRC = None                                      # the reference's src/ directory (argv[1], set in __main__)
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

from fashionvisualexpl_recommend_amd import synth  # noqa: E402  (numpy-only module)


def _import_reference():
    sys.modules.setdefault("tensorflow", types.ModuleType("tensorflow"))  # placeholder, never used
    sys.path.insert(0, REF_SRC)
    from dataset.dataset import DataLoader
    from recommender import Evaluator as ev
    return DataLoader, ev


def _ref_stream(DataLoader, workdir, name, batch_size, epochs):
    params = Namespace(dataset=name, validation=True, batch_size=batch_size, epochs=epochs, batch_eval=128)
    cwd = os.getcwd()
    os.chdir(os.path.join(workdir, "src"))          # reference paths are '../data/{0}/...'
    try:
        data = DataLoader(params=params)
        random.seed(0); np.random.seed(0)             # BPRMF.py:15-16 run at import, nothing consumes RNG before
        u, i, j = data.all_triple_batches()
    finally:
        os.chdir(cwd)
    arr = np.stack([np.array([int(x) for x in v], dtype=np.int64) for v in (u, i, j)])
    return data, arr


def main():
    DataLoader, ev = _import_reference()
    work = tempfile.mkdtemp(prefix="bprx_golden_")
    os.makedirs(os.path.join(work, "src"))
    droot = os.path.join(work, "data")
    out = {}

    # ---- case "tiny": 6 users x 9 items, ragged lists, bs=4, 2 epochs.  User 2 has NO training row: the
    # reference loader then shifts later rows into the gap (dataset.py:63-72, `u_ += 1` per boundary), which the
    # mirror must reproduce; the lists the REFERENCE loaded are stored as the expected loader output.
    tiny_train = [[0, 3, 5], [1, 2], [], [4, 6, 7, 8], [0, 8], [2, 3, 4, 5, 6]]
    tiny_val = [[1], [0], [3], [1], [5], [0]]
    tiny_test = [[2], [5], [7], [0], [6], [8]]
    synth.write_dataset(droot, "tiny", tiny_train, tiny_val, tiny_test, 9)
    data, arr = _ref_stream(DataLoader, work, "tiny", 4, 2)
    np.savez(os.path.join(HERE, "stream_tiny.npz"), uij=arr.astype(np.int32),
             meta=np.array([6, 9, 4, 2]))
    json.dump({"written_train": tiny_train, "val": tiny_val, "test": tiny_test, "num_items": 9,
               "loaded_train": data.training_list, "loaded_val": data.validation_list,
               "loaded_test": data.test_list},
              open(os.path.join(HERE, "dataset_tiny.json"), "w"))
    out["tiny"] = {"n": int(arr.shape[1])}

    # ---- case "short": N < batch_size  => (N//bs)*bs*epochs == 0, early-return never fires (dataset.py:89,109)
    data, arr = _ref_stream(DataLoader, work, "tiny", 64, 3)
    np.savez(os.path.join(HERE, "stream_short.npz"), uij=arr.astype(np.int32), meta=np.array([6, 9, 64, 3]))
    out["short"] = {"n": int(arr.shape[1])}

    # ---- case "c1": BASELINE config 1 shape (1K users x 2K items, 20 train/user, bs 256, 5 epochs) ---------
    tr, va, te = synth.make_interactions(1000, 2000, per_user=22, seed=2024)
    synth.write_dataset(droot, "c1", tr, va, te, 2000)
    data, arr = _ref_stream(DataLoader, work, "c1", 256, 5)
    assert data.training_list == tr
    sha = hashlib.sha256(np.ascontiguousarray(arr, dtype=np.int64).tobytes()).hexdigest()
    np.savez(os.path.join(HERE, "stream_c1_head.npz"), uij=arr[:, :4096].astype(np.int32),
             tail=arr[:, -256:].astype(np.int32), meta=np.array([1000, 2000, 256, 5]))
    out["c1"] = {"n": int(arr.shape[1]), "sha256_int64_3xN": sha}

    # ---- metric fixtures: reference Evaluator on seeded score matrices -----------------------------------------
    class _Scores:
        def __init__(self, a): self.a = a
        def numpy(self): return self.a.copy()

    class _Model:
        def __init__(self, data, a): self.data, self.a = data, a
        def predict_all(self): return _Scores(self.a)

    def run_eval(name, U, I, K, scores, with_val=True):
        params = Namespace(dataset=name, validation=with_val, batch_size=4, epochs=1, batch_eval=128)
        cwd = os.getcwd(); os.chdir(os.path.join(work, "src"))
        try:
            data = DataLoader(params=params)
            e = ev.Evaluator(_Model(data, scores), data, K)
            results = {}
            e.eval(1, results, "golden", 0)
            rec_path = os.path.join(work, "recs_%s_%d.tsv" % (name, with_val))
            e.store_recommendation(path=rec_path)
        finally:
            os.chdir(cwd)
        return results[1], open(rec_path).read()

    rs = np.random.RandomState(7)
    sc_tiny = rs.standard_normal((6, 9)).astype(np.float32)
    sc_tiny[3, :] = 0.25            # a full row of ties: exercises nlargest/>= tie rules
    sc_tiny[4, 1] = sc_tiny[4, 6]   # tie between a negative and the test item of user 4
    res, recs = run_eval("tiny", 6, 9, 3, sc_tiny)
    np.save(os.path.join(HERE, "eval_tiny_scores.npy"), sc_tiny)
    open(os.path.join(HERE, "eval_tiny_recs.tsv"), "w").write(recs)
    out["eval_tiny"] = {"K": 3, "results": res}
    # (validation=False cannot be captured: the reference itself raises TypeError at Evaluator.py:195-213,
    #  formatting the '0' string placeholders of :179 with %f.)

    sc_c1 = np.random.RandomState(11).standard_normal((1000, 2000)).astype(np.float32)
    res, recs = run_eval("c1", 1000, 2000, 10, sc_c1)
    out["eval_c1"] = {"K": 10, "score_seed": 11, "results": res,
                      "recs_sha256": hashlib.sha256(recs.encode()).hexdigest(),
                      "recs_head": recs.splitlines()[:20]}

    json.dump(out, open(os.path.join(HERE, "golden.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True)[:1500])


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: python tests/golden/gen_golden.py <reference>/src")
    REF_SRC = os.path.abspath(sys.argv[1])
    main()
