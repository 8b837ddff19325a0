"""Cost of influence explanations for every user's list (bprx_influence behind bprx_score_block + bprx_topk) on the C2 shape of
DESIGN.md: U = 100 000 users, I = 50 000 items, k = d = 64, D = 4 096, bf16 features, K = 20 per list, L = 5 entries per pair, 20
owned items x 4 negatives = 80 pairs per user.  Device work only: the download of the lists is the host's.

Each timing is the median of five windows with (min, max), all in one process, from device events around work that ends in a
synchronise:

  plain         every user block's bprx_score_block + bprx_topk with K = 20: what recs-* costs today (its lists are kept)
  because       bprx_because alone over the lists of ALL users at the same K and L, space 'both' (the --because pass)
  influence     bprx_influence alone over the lists of ALL users, on the handle's own rows; also on a VBPR handle of k + d = 128 +
                20 (the reference's default) and a BPRMF handle of k = 128

Beside `influence` its arithmetic per user: pairs n (n + 1) / 2 fma for the Hessian, n^3 / 6 for the factorisation, 2 K n^2 for the
solves and 2 K pairs n for the split (the pairs are formed twice).
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/influence_cost.py [--out profiles/influence_cost.json]"""
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
    ap.add_argument("--top", type=int, default=5, help="entries per pair (L)")
    ap.add_argument("--history", type=int, default=20, help="owned items per user")
    ap.add_argument("--negatives", type=int, default=4, help="pairs per owned item")
    ap.add_argument("--damp", type=float, default=1.0)
    ap.add_argument("--block", type=int, default=4096, help="users per score block (Evaluator.user_block)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "influence_cost.json"))
    a = ap.parse_args()
    nu, n, Df, topk, L, H, NEG = a.users, a.items, a.feat_dim, a.top_k, a.top, a.history, a.negatives
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, generator=g, device="cuda") * 2 - 1
    lim = lambda r, c: float(np.sqrt(6.0 / (r + c)))
    F = torch.randn((n, Df), generator=g, device="cuda").abs_()
    F *= torch.rand((n, Df), generator=g, device="cuda") < 0.5       # relu-like: about half zeros
    F = (F / F.max()).to(torch.bfloat16)

    def vbpr(k, d):
        t = dict(Gu=rnd(nu, k) * lim(nu, k), Gi=rnd(n, k) * lim(n, k), Bi=torch.zeros(n, device="cuda"), Tu=rnd(nu, d) * lim(nu, d),
                 E=rnd(Df, d) * lim(Df, d), Bp=rnd(Df) * lim(Df, 1), F=F)
        return Engine(model="vbpr", num_users=nu, num_items=n, embed_k=k, embed_d=d, feat_dim=Df, feat_dtype="bf16", optimizer="sgd",
                      lr=0.05, reg=0.0, max_batch=4096).bind(**t)

    e = vbpr(K, DD)
    owned = torch.randint(0, n, (nu * H,), generator=g, device="cuda", dtype=torch.int32)
    train = (torch.arange(nu + 1, dtype=torch.int64, device="cuda") * H, owned)   # the masked training items ARE the history
    pair_ptr = torch.arange(nu + 1, dtype=torch.int64, device="cuda") * (H * NEG)
    pos = owned.repeat_interleave(NEG).contiguous()
    neg = torch.randint(0, n, (nu * H * NEG,), generator=g, device="cuda", dtype=torch.int32)
    blocks = [(u0, min(nu, u0 + a.block)) for u0 in range(0, nu, a.block)]
    scores = torch.empty((a.block, n), dtype=torch.float32, device="cuda")
    lists = torch.empty((nu, topk), dtype=torch.int32, device="cuda")
    results = []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)

    def ranked():
        for u0, u1 in blocks:
            lists[u0:u1] = e.topk(u0, u1, e.score_block(u0, u1, out=scores[:u1 - u0]), train, topk)[0]

    r = {"case": "plain", "users": nu, "items": n, "top_k": topk, "history": H, "blocks": len(blocks)}
    r.update(windows(ranked, 1))
    emit(r)
    plain_ms = r["ms"]
    rn = e.sim_rnorm("both")                                        # (P is made current here, once per parameter state)
    r = {"case": "because", "space": "both", "width": K + DD, "users": nu, "top_k": topk, "top": L, "history": H}
    r.update(windows(lambda: e.because("both", rn, lists, train, L), 3))
    r.update(share_of_plain=round(r["ms"] / plain_ms, 4))
    emit(r)
    because_ms = r["ms"]

    def influence(eng, tag):
        w, m = eng.k + eng.d, H * NEG
        Gu, Tu = eng.t["Gu"], (eng.t["Tu"] if eng.d else None)
        call = lambda: eng.influence(Gu, Tu, pair_ptr, pos, neg, NEG, lists, L, reg=0.0, damp=a.damp)
        flagged = int(call()["flag"].sum().item())
        r = {"case": "influence", "handle": tag, "width": w, "users": nu, "top_k": topk, "top": L, "history": H, "negatives": NEG,
             "pairs": m, "damp": a.damp, "flagged_rows": flagged}
        r.update(windows(call, 3))
        r.update(fma_per_user={"hessian": m * w * (w + 1) // 2, "cholesky": w ** 3 // 6, "solves": 2 * topk * w * w,
                               "split": 2 * topk * m * w})
        return r

    r = influence(e, "vbpr k = d = 64")
    r.update(ratio_to_plain=round(r["ms"] / plain_ms, 4), ratio_to_because=round(r["ms"] / because_ms, 4))
    emit(r)
    e.sync_check()
    e.close()
    e = vbpr(128, 20)
    emit(influence(e, "vbpr k = 128, d = 20"))
    e.sync_check()
    e.close()
    e = Engine(model="bprmf", num_users=nu, num_items=n, embed_k=128, optimizer="sgd", lr=0.05, reg=0.0, max_batch=4096)
    e.bind(rnd(nu, 128) * lim(nu, 128), rnd(n, 128) * lim(n, 128), torch.zeros(n, device="cuda"))
    emit(influence(e, "bprmf k = 128"))
    e.sync_check()
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
