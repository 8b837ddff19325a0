"""Cost of "because you own X" for every user's list (bprx_because behind bprx_score_block + bprx_topk) on the C2 shape of
DESIGN.md: U = 100 000 users, I = 50 000 items, k = d = 64, D = 4 096, bf16 features, K = 20 per list, L = 5 owned items per pair,
20 history items per user.  Device work only: the download of the lists is the host's.

Each timing is the median of five windows with (min, max), all in one process, from device events around work that ends in a
synchronise:

  plain         every user block's bprx_score_block + bprx_topk with K = 20: what recs-* costs today (its lists are kept)
  because       bprx_because alone over the lists of ALL users, per space

Beside `because` the byte bound of DESIGN.md: a list gathers its K item rows and its H history rows of w floats once,
n (K + H) w 4 bytes against 8 TB/s -- the optimistic HBM figure, although the catalogue's z (13-26 MB) stays in the Infinity
Cache and the rows come from there.
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/because_cost.py [--out profiles/because_cost.json]"""
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
    ap.add_argument("--top", type=int, default=5, help="owned items per pair (L)")
    ap.add_argument("--history", type=int, default=20, help="history items per user")
    ap.add_argument("--spaces", nargs="+", default=["visual", "both", "latent"])
    ap.add_argument("--block", type=int, default=4096, help="users per score block (Evaluator.user_block)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "because_cost.json"))
    a = ap.parse_args()
    nu, n, Df, topk, L, H = a.users, a.items, a.feat_dim, a.top_k, a.top, a.history
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
    train = (torch.arange(nu + 1, dtype=torch.int64, device="cuda") * H,          # the masked training items ARE the history
             torch.randint(0, n, (nu * H,), generator=g, device="cuda", dtype=torch.int32))
    blocks = [(u0, min(nu, u0 + a.block)) for u0 in range(0, nu, a.block)]
    scores = torch.empty((a.block, n), dtype=torch.float32, device="cuda")
    lists = torch.empty((nu, topk), dtype=torch.int32, device="cuda")
    results = []

    def ranked():
        for u0, u1 in blocks:
            lists[u0:u1] = e.topk(u0, u1, e.score_block(u0, u1, out=scores[:u1 - u0]), train, topk)[0]

    r = {"case": "plain", "users": nu, "items": n, "top_k": topk, "history": H, "blocks": len(blocks)}
    r.update(windows(ranked, 1))
    print(json.dumps(r), flush=True)
    results.append(r)
    plain_ms = r["ms"]
    for space in a.spaces:
        w = {"latent": K, "visual": DD, "both": K + DD}[space]
        rn = e.sim_rnorm(space)                                     # (P is made current here, once per parameter state)
        r = {"case": "because", "space": space, "width": w, "users": nu, "top_k": topk, "top": L, "history": H}
        r.update(windows(lambda: e.because(space, rn, lists, train, L), 3))
        bytes_ms = nu * (topk + H) * w * 4.0 / HBM_BYTES_PER_S * 1e3
        r.update(bytes_bound_ms=round(bytes_ms, 4), fraction_of_bytes_bound=round(bytes_ms / r["ms"], 3),
                 fma_per_list=topk * H * w, share_of_plain=round(r["ms"] / plain_ms, 4))
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
