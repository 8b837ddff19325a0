"""Cost of one audience pass over the whole catalogue (bprx_audience_block + bprx_topk_rows_masked) against the plain ranking pass
(bprx_score_block + bprx_topk, store_recommendation's loop) on the C2 shape of DESIGN.md: U = 100 000 users, I = 50 000 items,
k = d = 64, D = 4 096, bf16 features, K = 20 per list, 20 training items per user.  Both passes produce the same 5 * 10^9 scores,
one user-major in blocks of users, one item-major in blocks of items (ranking.rows_per_block cuts a block of 100 000-wide rows to
1 342 of them).  Device work only: the download of the lists is the host's.

Each timing is the median of five windows with (min, max), all in one process, from device events around work that ends in a
synchronise:

  plain           every user block's bprx_score_block + bprx_topk with K = 20: what recs-* costs today
  audience        every item block's bprx_audience_block + bprx_topk_rows_masked with K = 20, the owners of each item masked
  audience_block  every item block's bprx_audience_block, nothing else
  ranking         every item block's bprx_topk_rows_masked on a block of scores that is already there
  plain_block / plain_ranking   the same split of the plain pass

Prints one JSON line per case and writes them all to --out.
Usage: python scripts/audience_cost.py [--out profiles/audience_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402
from fashionvisualexpl_recommend_amd.ranking import blocks  # noqa: E402

U, I, K, DD, D = 100_000, 50_000, 64, 64, 4096


def windows(fn, reps, passes=5):
    fn()                                                            # warm-up: code objects, the allocator's blocks, clocks
    torch.cuda.synchronize()
    out = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return {"ms": round(float(np.median(out)), 4), "ms_min_max": [round(min(out), 4), round(max(out), 4)], "passes_per_window": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=U, help="users (a rehearsal takes fewer)")
    ap.add_argument("--items", type=int, default=I)
    ap.add_argument("--feat_dim", type=int, default=D)
    ap.add_argument("--top_k", type=int, default=20)
    ap.add_argument("--history", type=int, default=20, help="training items per user")
    ap.add_argument("--block", type=int, default=4096, help="rows per block before the width cuts it (Evaluator.user_block)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audience_cost.json"))
    a = ap.parse_args()
    nu, n, Df, topk, H = a.users, a.items, a.feat_dim, a.top_k, a.history
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, generator=g, device="cuda") * 2 - 1
    lim = lambda r, c: float(np.sqrt(6.0 / (r + c)))
    F = torch.randn((n, Df), generator=g, device="cuda").abs_()
    F *= torch.rand((n, Df), generator=g, device="cuda") < 0.5       # relu-like: about half zeros
    t = dict(Gu=rnd(nu, K) * lim(nu, K), Gi=rnd(n, K) * lim(n, K), Bi=torch.zeros(n, device="cuda"), Tu=rnd(nu, DD) * lim(nu, DD),
             E=rnd(Df, DD) * lim(Df, DD), Bp=rnd(Df) * lim(Df, 1), F=(F / F.max()).to(torch.bfloat16))
    del F
    e = Engine(model="vbpr", num_users=nu, num_items=n, embed_k=K, embed_d=DD, feat_dim=Df, feat_dtype="bf16", optimizer="sgd",
               lr=0.05, reg=0.0, max_batch=4096).bind(**t)
    items = torch.randint(0, n, (nu * H,), generator=g, device="cuda", dtype=torch.int32)
    train = (torch.arange(nu + 1, dtype=torch.int64, device="cuda") * H, items)
    # the owners of every item: the same pairs, by item (a user that drew an item twice is named twice: harmless)
    order = torch.sort(items.long(), stable=True)[1]
    own_users = torch.arange(nu, device="cuda").repeat_interleave(H)[order].to(torch.int32)
    own_ptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    own_ptr[1:] = torch.cumsum(torch.bincount(items.long(), minlength=n), 0)
    del order
    ublocks = list(blocks(nu, a.block))                              # store_recommendation's blocks of users
    iblocks = list(blocks(n, a.block, nu))                           # audience's blocks of items, cut by the row width
    rows_u, rows_i = max(b1 - b0 for b0, b1 in ublocks), max(b1 - b0 for b0, b1 in iblocks)
    buf = torch.empty(max(rows_u * n, rows_i * nu), dtype=torch.float32, device="cuda")
    ub = lambda u0, u1: buf[:(u1 - u0) * n].view(u1 - u0, n)
    ib = lambda q0, q1: buf[:(q1 - q0) * nu].view(q1 - q0, nu)
    e.score_block(0, 1)                                              # (P is made current here, once per parameter state)
    results = []

    def case(name, fn, reps, **kw):
        r = {"case": name, "users": nu, "items": n, "top_k": topk, "history": H}
        r.update(kw)
        r.update(windows(fn, reps))
        if results:
            r["ratio_to_plain"] = round(r["ms"] / results[0]["ms"], 4)
        print(json.dumps(r), flush=True)
        results.append(r)

    def plain():
        for u0, u1 in ublocks:
            e.topk(u0, u1, e.score_block(u0, u1, out=ub(u0, u1)), train, topk)

    def audience():
        for q0, q1 in iblocks:
            e.topk_rows_masked(e.audience_block(q0, q1, out=ib(q0, q1)), (own_ptr[q0:q1 + 1], own_users), topk)

    def plain_block():
        for u0, u1 in ublocks:
            e.score_block(u0, u1, out=ub(u0, u1))

    def audience_block():
        for q0, q1 in iblocks:
            e.audience_block(q0, q1, out=ib(q0, q1))

    def plain_ranking():                                             # (the block is masked after the first pass: the same work)
        for u0, u1 in ublocks:
            e.topk(u0, u1, ub(u0, u1), train, topk)

    def ranking():
        for q0, q1 in iblocks:
            e.topk_rows_masked(ib(q0, q1), (own_ptr[q0:q1 + 1], own_users), topk)

    case("plain", plain, 1, blocks=len(ublocks), rows_per_block=rows_u, row_width=n)
    case("audience", audience, 1, blocks=len(iblocks), rows_per_block=rows_i, row_width=nu)
    case("plain_block", plain_block, 1, blocks=len(ublocks))
    case("audience_block", audience_block, 1, blocks=len(iblocks))
    plain_block()
    case("plain_ranking", plain_ranking, 1, rows=nu, row_width=n)
    audience_block()
    case("ranking", ranking, 1, rows=n, row_width=nu)
    e.sync_check()
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
