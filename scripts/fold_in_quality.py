"""What folding in buys a user the model was not trained on, on the clustered synthetic data (synth.make_interactions_clustered).

BPRMF is trained on users [0, U') with the device sampler; the remaining users are folded in from their TRAINING lists
(models.draw_fold_pairs -> Engine.fold_in, zero start rows) and ranked over the catalogue with their histories masked
(score_rows_block).  HR@K / NDCG@K of their held-out (validation + test) items, next to the zero-row start -- which ranks every
user by Bi alone -- and to the trained users' own figures as the ceiling.
Usage: python scripts/fold_in_quality.py [--out profiles/fold_in_quality.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd import synth  # noqa: E402
from fashionvisualexpl_recommend_amd.engine import Engine, PhiloxSampler  # noqa: E402
from fashionvisualexpl_recommend_amd.models import draw_fold_pairs  # noqa: E402


def metrics(scores, hist, held, K):
    """(HR@K, NDCG@K) of the held-out items, each ranked against the items outside the history (one relevant item at a time)."""
    hr, nd, cnt = 0.0, 0.0, 0
    for r in range(scores.shape[0]):
        row = scores[r].copy()
        row[hist[r]] = -np.inf
        for it in held[r]:
            other = row.copy()
            other[[x for x in held[r] if x != it]] = -np.inf
            rank = int((other > other[it]).sum())
            hr += rank < K
            nd += 1.0 / np.log2(rank + 2) if rank < K else 0.0
            cnt += 1
    return round(hr / cnt, 4), round(nd / cnt, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=3000)
    ap.add_argument("--trained", type=int, default=2400)
    ap.add_argument("--items", type=int, default=1000)
    ap.add_argument("--embed_k", type=int, default=32)
    ap.add_argument("--train_steps", type=int, default=3000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--fold_steps", type=int, default=30)
    ap.add_argument("--negatives", type=int, default=4)
    ap.add_argument("--top_k", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_in_quality.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    U, Ut, I, k = a.users, a.trained, a.items, a.embed_k
    tr, va, te = synth.make_interactions_clustered(U, I, per_user=22, seed=7)
    rs = np.random.RandomState(0)
    e = Engine(model="bprmf", num_users=Ut, num_items=I, embed_k=k, optimizer="sgd", lr=0.05, reg=1e-4, max_batch=a.batch)
    e.bind(synth.glorot_uniform(rs, Ut, k), synth.glorot_uniform(rs, I, k), np.zeros(I, np.float32))
    smp = PhiloxSampler(tr[:Ut], I, seed=1).feeds(e)
    for _ in range(a.train_steps):
        e.step(*smp.sample(a.batch), want_loss=False)
    e.sync_check()
    held = [va[u] + te[u] for u in range(U)]
    out = {"data": "make_interactions_clustered(%d, %d, per_user=22, seed=7)" % (U, I), "model": "bprmf", "embed_k": k,
           "trained_users": Ut, "folded_users": U - Ut, "train_steps": a.train_steps, "batch": a.batch, "K": a.top_k,
           "fold": {"steps": a.fold_steps, "negatives": a.negatives, "optimizer": "sgd", "lr": 0.05, "reg": 1e-4}}
    hr, nd = metrics(e.score_block(0, Ut).cpu().numpy(), tr[:Ut], held[:Ut], a.top_k)
    out["trained_users_hr_ndcg"] = [hr, nd]
    hist = tr[Ut:]
    n = len(hist)
    ptr, pos, neg = draw_fold_pairs(hist, I, a.negatives, seed=0)
    Gu = torch.zeros((n, k), device="cuda")
    hr, nd = metrics(e.score_rows_block(Gu, None, 0, n).cpu().numpy(), hist, held[Ut:], a.top_k)
    out["zero_rows_hr_ndcg"] = [hr, nd]
    loss = e.fold_in(ptr, pos, neg, a.fold_steps, Gu, None, lr=0.05, reg=1e-4, optimizer="sgd")
    hr, nd = metrics(e.score_rows_block(Gu, None, 0, n).cpu().numpy(), hist, held[Ut:], a.top_k)
    out["folded_in_hr_ndcg"] = [hr, nd]
    out["mean_loss_per_pair_at_last_step"] = round(float(loss.sum().item()) / max(1, len(pos)), 4)
    out["random_ranking_hr"] = round(a.top_k / (I - 20), 4)
    e.sync_check()
    e.close()
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
