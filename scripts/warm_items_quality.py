"""What a new item's first buyers buy, on the clustered synthetic data (synth.make_interactions_clustered) with features that carry
the item's cluster (|prototype of the cluster + noise|: a picture says something about who buys the item, not everything).

VBPR is trained on the catalogue without a held-out tenth of the items (every tenth id; the lists lose those items).  Each held-out
item is then fitted from m = 2, 5 and 20 of its buyers (models.draw_item_fold_pairs -> Engine.fold_in_items, zero start rows,
adam_tf23) and its audience ranked over all users with those m buyers masked (Engine.audience_warm_block: the ranking
model.audience_warm lists).  HR@K / NDCG@K of the item's REMAINING buyers, one relevant user at a time against the users that are
neither fold buyers nor other remaining buyers, next to
  floor    the visual score alone (audience_block on the projected rows: what audience_new ranks by), same masks;
  ceiling  the same items trained IN the catalogue, a run of its own in which a held-out item keeps the interactions of exactly
           those m buyers (audience_block), same masks.
Items with fewer than m + 1 buyers are left out of the row for m.
Usage: python scripts/warm_items_quality.py [--out profiles/warm_items_quality.json]"""
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
from fashionvisualexpl_recommend_amd.models import draw_item_fold_pairs  # noqa: E402

CLUSTERS, SEED = 20, 7


def features(num_items, dim, noise, seed):
    """[I, dim] in [0, 1]: |prototype of the item's cluster + noise * N(0, 1)| / max; the clusters are those of
    make_interactions_clustered(seed=SEED), whose first draw they are."""
    cluster = np.random.RandomState(SEED).randint(CLUSTERS, size=num_items)
    rs = np.random.RandomState(seed)
    proto = rs.standard_normal((CLUSTERS, dim))
    f = np.abs(proto[cluster] + noise * rs.standard_normal((num_items, dim))).astype(np.float32)
    return f / f.max()


def train(lists, num_items, F, a, seed):
    U, k, d = len(lists), a.embed_k, a.embed_d
    rs = np.random.RandomState(seed)
    e = Engine(model="vbpr", num_users=U, num_items=num_items, embed_k=k, embed_d=d, feat_dim=F.shape[1], feat_dtype="fp32",
               optimizer="sgd", lr=0.05, reg=1e-4, max_batch=a.batch)
    e.bind(synth.glorot_uniform(rs, U, k), synth.glorot_uniform(rs, num_items, k), np.zeros(num_items, np.float32),
           synth.glorot_uniform(rs, U, d), F, synth.glorot_uniform(rs, F.shape[1], d), synth.glorot_uniform(rs, F.shape[1], 1).reshape(-1))
    smp = PhiloxSampler(lists, num_items, seed=1).feeds(e)
    for _ in range(a.train_steps):
        e.step(*smp.sample(a.batch), want_loss=False)
    e.sync_check()
    return e


def metrics(rows, fold, rest, K):
    """(HR@K, NDCG@K, relevant users) of the remaining buyers rest[j] in the score rows [n, U], the fold buyers masked."""
    hr, nd, cnt = 0.0, 0.0, 0
    for j in range(rows.shape[0]):
        if not rest[j]:
            continue
        row = rows[j].astype(np.float64).copy()
        row[fold[j]] = -np.inf
        sc = row[rest[j]]
        row[rest[j]] = -np.inf
        for s in sc:
            rank = int((row > s).sum())
            hr += rank < K
            nd += 1.0 / np.log2(rank + 2) if rank < K else 0.0
            cnt += 1
    return round(hr / max(cnt, 1), 4), round(nd / max(cnt, 1), 4), cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=3000)
    ap.add_argument("--items", type=int, default=1000)
    ap.add_argument("--feat_dim", type=int, default=64)
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--embed_k", type=int, default=32)
    ap.add_argument("--embed_d", type=int, default=16)
    ap.add_argument("--train_steps", type=int, default=3000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--buyers", type=int, nargs="+", default=[2, 5, 20])
    ap.add_argument("--fold_steps", type=int, default=30)
    ap.add_argument("--negatives", type=int, default=4)
    ap.add_argument("--top_k", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warm_items_quality.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    U, I, K = a.users, a.items, a.top_k
    tr, _, _ = synth.make_interactions_clustered(U, I, per_user=22, clusters=CLUSTERS, seed=SEED)
    F = features(I, a.feat_dim, a.noise, seed=11)
    held = np.arange(9, I, 10)                                          # every tenth item
    cat = np.setdiff1d(np.arange(I), held)
    new_id = np.full(I, -1, np.int64)
    new_id[cat] = np.arange(cat.size)
    is_held = np.zeros(I, bool)
    is_held[held] = True
    lists_cat = [[int(new_id[i]) for i in l if not is_held[i]] for l in tr]
    owners = [[] for _ in range(I)]
    for u, l in enumerate(tr):
        for i in l:
            owners[i].append(u)
    rs = np.random.RandomState(3)
    order = [list(rs.permutation(owners[int(j)])) for j in held]      # each held-out item's buyers in a random arrival order
    e = train(lists_cat, cat.size, F[cat], a, seed=0)
    Pn = e.project_rows(F[held])
    n = held.size
    out = {"data": "make_interactions_clustered(%d, %d, per_user=22, clusters=%d, seed=%d), training lists" % (U, I, CLUSTERS, SEED),
           "features": "|cluster prototype + %g N(0,1)| / max, %d columns" % (a.noise, a.feat_dim), "model": "vbpr",
           "embed_k": a.embed_k, "embed_d": a.embed_d, "train_steps": a.train_steps, "batch": a.batch, "held_out_items": int(n),
           "mean_buyers_per_held_out_item": round(float(np.mean([len(o) for o in order])), 1), "K": K, "users_ranked": U,
           "fold": {"steps": a.fold_steps, "negatives": a.negatives, "optimizer": "adam_tf23", "lr": 0.05, "reg": 1e-4}, "rows": []}
    visual = e.audience_block(0, n, Pn).cpu().numpy()
    for m in a.buyers:
        ok = [len(o) > m for o in order]
        fold = [o[:m] if good else [] for o, good in zip(order, ok)]
        rest = [o[m:] if good else [] for o, good in zip(order, ok)]
        row = {"buyers_known": m, "items_evaluated": int(sum(ok))}
        row["visual_only_hr_ndcg"] = list(metrics(visual, fold, rest, K)[:2])
        ptr, user, other, role = draw_item_fold_pairs(fold, lists_cat, cat.size, a.negatives, seed=0)
        Gi, Bi = torch.zeros((n, a.embed_k), device="cuda"), torch.zeros(n, device="cuda")
        loss = e.fold_in_items(ptr, user, other, role, a.fold_steps, Gi, Bi, Pn, lr=0.05, reg=1e-4, optimizer="adam_tf23")
        warm = e.audience_warm_block(Gi, Bi, Pn, 0, n).cpu().numpy()
        hr, nd, cnt = metrics(warm, fold, rest, K)
        row["warm_hr_ndcg"], row["relevant_users"] = [hr, nd], cnt
        row["mean_loss_per_pair_at_last_step"] = round(float(loss.sum().item()) / max(1, len(user)), 4)
        # the ceiling: the held-out items in the catalogue, trained with the interactions of exactly these buyers
        keep = [set() for _ in range(U)]
        for j, f in zip(held, fold):
            for u in f:
                keep[u].add(int(j))
        lists_full = [[i for i in l if not is_held[i] or i in keep[u]] for u, l in enumerate(tr)]
        ec = train(lists_full, I, F, a, seed=0)
        full = ec.audience_block(0, I).cpu().numpy()[held]
        ec.close()
        row["trained_in_catalogue_hr_ndcg"] = list(metrics(full, fold, rest, K)[:2])
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
    out["random_ranking_hr"] = round(K / U, 4)
    e.sync_check()
    e.close()
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
