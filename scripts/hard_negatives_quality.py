"""What training on hard negatives does to the ranking, on the clustered synthetic data (synth.make_interactions_clustered, 3 000
users x 3 000 items) through the training loop of the CLI (BPRMF.train / VBPR.train with sampler = philox): test HR@20 / nDCG@20
after every epoch for C = 1 (the uniform epoch walk) and --hard_negatives 2, 4, 8, same seeds, learning rate, batch size and
epochs.  VBPR gets features that carry the item's cluster (|prototype of the cluster + noise|, as scripts/warm_items_quality.py),
and for one C a second run with --hard_refresh of a quarter epoch (BPRMF has no snapshot to refresh).

The held-out validation and test items are among the candidates, as they are among the uniform negatives (the reference excludes
neither, dataset.py:93-107); a sampler that looks for the best-scored candidate finds them more often than a uniform one, which
pushes exactly the items the metric looks for down.  Whatever comes out is recorded, a loss included.
Usage: python scripts/hard_negatives_quality.py [--out profiles/hard_negatives_quality.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd import configs, synth  # noqa: E402

CLUSTERS, SEED = 20, 7


def features(num_items, dim, noise, seed):
    """[I, dim]: |prototype of the item's cluster + noise * N(0, 1)|; the clusters are those of make_interactions_clustered(seed=SEED),
    whose first draw they are."""
    cluster = np.random.RandomState(SEED).randint(CLUSTERS, size=num_items)
    rs = np.random.RandomState(seed)
    proto = rs.standard_normal((CLUSTERS, dim))
    return np.abs(proto[cluster] + noise * rs.standard_normal((num_items, dim))).astype(np.float32)


def run(rec, a, hard, refresh):
    from fashionvisualexpl_recommend_amd.dataset import DataLoader
    from fashionvisualexpl_recommend_amd.models import BPRMF, VBPR
    p = Namespace(dataset="hnq", validation=True, batch_size=a.batch, epochs=a.epochs, batch_eval=1024, embed_k=a.embed_k,
                  embed_d=a.embed_d, lr=a.lr, reg=a.reg, top_k=a.top_k, verbose=-1, restore_epochs=1, rec=rec, best_metric="ndcg",
                  optimizer="adam_tf23", init_seed=0, dtype="bf16", cnn_model="vgg19", output_layer="fc2", sampler="philox",
                  hard_negatives=hard, hard_refresh=refresh)
    with contextlib.redirect_stdout(io.StringIO()):
        model = (VBPR if rec == "vbpr" else BPRMF)(DataLoader(p), p)
        res = model.train()
        model.engine.sync_check()
        model.engine.close()
    return {"rec": rec, "candidates": max(hard, 1), "hard_refresh": refresh,
            "hr_t": [round(float(res[e]["hr_t"]), 4) for e in sorted(res)], "ndcg_t": [round(float(res[e]["ndcg_t"]), 4) for e in sorted(res)],
            "hr_v": [round(float(res[e]["hr_v"]), 4) for e in sorted(res)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=3000)
    ap.add_argument("--items", type=int, default=3000)
    ap.add_argument("--feat_dim", type=int, default=256)
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--embed_k", type=int, default=32)
    ap.add_argument("--embed_d", type=int, default=16)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=12)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--reg", type=float, default=1e-3)
    ap.add_argument("--top_k", type=int, default=20)
    ap.add_argument("--candidates", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--refresh_c", type=int, default=4, help="the C that also runs with --hard_refresh of a quarter epoch (VBPR)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hard_negatives_quality.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    U, I = a.users, a.items
    tr, va, te = synth.make_interactions_clustered(U, I, per_user=22, clusters=CLUSTERS, seed=SEED)
    steps_per_epoch = sum(len(l) for l in tr) // a.batch
    out = {"data": "make_interactions_clustered(%d, %d, per_user=22, clusters=%d, seed=%d)" % (U, I, CLUSTERS, SEED),
           "features": "|cluster prototype + %g N(0,1)|, %d columns, bf16" % (a.noise, a.feat_dim), "K": a.top_k,
           "optimizer": "adam_tf23", "lr": a.lr, "reg": a.reg, "batch": a.batch, "epochs": a.epochs, "steps_per_epoch": steps_per_epoch,
           "embed_k": a.embed_k, "embed_d": a.embed_d, "random_ranking_hr": round(a.top_k / I, 4),
           "note": "validation and test items are among the candidates (and among the uniform negatives)", "rows": []}
    with tempfile.TemporaryDirectory() as tmp:
        synth.write_dataset(tmp, "hnq", tr, va, te, I, features=features(I, a.feat_dim, a.noise, seed=11))
        configs.set_roots(tmp, os.path.join(tmp, "results"))
        for rec in ("bprmf", "vbpr"):
            for c in a.candidates:
                row = run(rec, a, 0 if c == 1 else c, 0)
                print(json.dumps(row), flush=True)
                out["rows"].append(row)
        row = run("vbpr", a, a.refresh_c, max(1, steps_per_epoch // 4))
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
