"""Cost of diversified lists for every user (bprx_diversify behind bprx_score_block + bprx_topk) on the C2 shape of DESIGN.md:
U = 100 000 users, I = 50 000 items, k = d = 64, D = 4 096, bf16 features, K = 20 per list.  Device work only: the download of the
lists and their upload as pools (ranking.diversify_rows) are the host's.

Each timing is the median of five windows with (min, max), all in one process, from device events around work that ends in a
synchronise:

  plain         every user block's bprx_score_block + bprx_topk with K = 20: what recs-* costs today
  pool          the same with K = N (the candidate pool), N = 100 and 256
  diversify     bprx_diversify alone over the pools of ALL users, per space and pool size, theta = 0.5

Beside `diversify` the two bounds of DESIGN.md.  Rows: a list gathers N rows of w floats once (LDS form) or K - 1 times (global
form); n N w 4 bytes against 8 TB/s is the optimistic HBM figure, although the catalogue's z (13-26 MB) stays in the Infinity
Cache and the rows come from there.  Rounds: a list is K sequential rounds, and a CU holds only as many lists as its LDS
(160 KiB) and its wave slots allow, so the pass cannot be faster than ceil(n / lists in flight) x K x (one round's latency); the
round latency is reported as measured (ms x lists in flight / n / K), not assumed.
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/diversify_cost.py [--out profiles/diversify_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402

U, I, K, DD, D = 100_000, 50_000, 64, 64, 4096
HBM_BYTES_PER_S = 8e12
CUS, LDS_PER_CU, LDS_FORM_MAX, WAVES_PER_CU, WAVES_PER_LIST = 256, 160 * 1024, 63 * 1024, 32, 4


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
    ap.add_argument("--pools", nargs="+", type=int, default=[100, 256])
    ap.add_argument("--spaces", nargs="+", default=["visual", "both", "latent"])
    ap.add_argument("--block", type=int, default=4096, help="users per score block (Evaluator.user_block)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diversify_cost.json"))
    a = ap.parse_args()
    nu, n, Df, topk = a.users, a.items, a.feat_dim, a.top_k
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
    per_user = 8                                                    # masked training items per user
    train = (torch.arange(nu + 1, dtype=torch.int64, device="cuda") * per_user,
             torch.randint(0, n, (nu * per_user,), generator=g, device="cuda", dtype=torch.int32))
    blocks = [(u0, min(nu, u0 + a.block)) for u0 in range(0, nu, a.block)]
    scores = torch.empty((a.block, n), dtype=torch.float32, device="cuda")
    results = []

    def ranked(kq, keep=None):
        for u0, u1 in blocks:
            idx, val, _ = e.topk(u0, u1, e.score_block(u0, u1, out=scores[:u1 - u0]), train, kq)
            if keep is not None:
                keep[0][u0:u1], keep[1][u0:u1] = idx, val

    r = {"case": "plain", "users": nu, "items": n, "top_k": topk, "blocks": len(blocks)}
    r.update(windows(lambda: ranked(topk), 1))
    print(json.dumps(r), flush=True)
    results.append(r)
    plain_ms = r["ms"]
    pools = {}
    for N in a.pools:
        pools[N] = (torch.empty((nu, N), dtype=torch.int32, device="cuda"), torch.empty((nu, N), dtype=torch.float32, device="cuda"))
        r = {"case": "pool", "users": nu, "items": n, "pool": N, "blocks": len(blocks)}
        r.update(windows(lambda: ranked(N, pools[N]), 1))
        r["times_plain"] = round(r["ms"] / plain_ms, 2)
        print(json.dumps(r), flush=True)
        results.append(r)
    for space in a.spaces:
        w = {"latent": K, "visual": DD, "both": K + DD}[space]
        rn = e.sim_rnorm(space)                                     # (P is made current here, once per parameter state)
        for N in a.pools:
            pi, pv = pools[N]
            lds_bytes = N * (w | 1) * 4 + N * 8
            form = "lds" if lds_bytes <= LDS_FORM_MAX else "global"
            per_cu = min(WAVES_PER_CU // WAVES_PER_LIST, LDS_PER_CU // max(lds_bytes if form == "lds" else N * 8, 1))
            in_flight = CUS * per_cu
            r = {"case": "diversify", "space": space, "width": w, "users": nu, "pool": N, "top_k": topk, "theta": 0.5, "rows": form,
                 "lds_bytes_per_list": lds_bytes if form == "lds" else N * 8, "lists_in_flight": in_flight}
            r.update(windows(lambda: e.diversify(space, rn, pi, pv, topk, 0.5), 3))
            gathers = 1 if form == "lds" else topk - 1
            rows_ms = nu * N * w * 4.0 * gathers / HBM_BYTES_PER_S * 1e3
            r.update(rows_bound_ms=round(rows_ms, 4), fraction_of_rows_bound=round(rows_ms / r["ms"], 3),
                     round_us_measured=round(r["ms"] * 1e3 * min(in_flight, nu) / nu / topk, 3),
                     times_plain=round(r["ms"] / plain_ms, 3))
            print(json.dumps(r), flush=True)
            results.append(r)
    e.sync_check()
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
