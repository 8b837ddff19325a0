"""Cost of the per-column explanation (bprx_feat_explain) next to the score it explains (bprx_score_pairs), on the C2 shape of
DESIGN.md: U = 100 000, I = 50 000, k = d = 64, D = 4 096.  Every user is explained for 20 items (2 000 000 pairs) in blocks of
--block users grouped by user, one call per block; bf16 and fp32 features, top = 5 and 32, with and without the map, and one pass
over the same pairs in shuffled order.  bprx_score_pairs runs over the same blocks in the same process.  ms = the median of five
timed windows (one pass over all pairs each, after a warm-up pass), with (min, max).  Beside it the bytes bound of the pass:
n D sizeof(feature) / 8 TB/s for the feature rows, plus n D 4 bytes when the map is written, and the achieved fraction of it.
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/feat_explain_cost.py [--block 4096] [--out profiles/feat_explain_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402

U, I, K, DD, D, PER_USER = 100_000, 50_000, 64, 64, 4096, 20
HBM_BYTES_PER_S = 8e12


def windows(fn, passes=5):
    fn()                                                            # warm-up: code objects, the allocator's blocks, clocks
    torch.cuda.synchronize()
    out = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"ms": round(float(np.median(out)), 3), "ms_min_max": [round(min(out), 3), round(max(out), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=4096, help="users per call")
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--tops", nargs="+", type=int, default=[5, 32])
    ap.add_argument("--users", type=int, default=U, help="users explained (a rehearsal takes fewer)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "feat_explain_cost.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, generator=g, device="cuda") * 2 - 1
    lim = lambda r, c: float(np.sqrt(6.0 / (r + c)))
    t = dict(Gu=rnd(U, K) * lim(U, K), Gi=rnd(I, K) * lim(I, K), Bi=torch.zeros(I, device="cuda"), Tu=rnd(U, DD) * lim(U, DD),
             E=rnd(D, DD) * lim(D, DD), Bp=rnd(D) * lim(D, 1))
    F32 = torch.randn((I, D), generator=g, device="cuda").abs_()
    F32 *= torch.rand((I, D), generator=g, device="cuda") < 0.5     # relu-like: about half zeros
    F32 /= F32.max()
    items = torch.randint(0, I, (U, PER_USER), generator=g, device="cuda", dtype=torch.int32)
    n_users = min(a.users, U)
    pairs = n_users * PER_USER
    results = []
    for dtype in a.dtypes:
        esz = 4 if dtype == "fp32" else 2
        e = Engine(model="vbpr", num_users=U, num_items=I, embed_k=K, embed_d=DD, feat_dim=D, feat_dtype=dtype, optimizer="sgd",
                   lr=0.05, reg=0.0, max_batch=a.block * PER_USER).bind(**t, F=F32)
        blocks = []
        for u0 in range(0, n_users, a.block):
            u = torch.arange(u0, min(n_users, u0 + a.block), dtype=torch.int32, device="cuda")
            blocks.append((u.repeat_interleave(PER_USER), items[u0:u0 + u.numel()].reshape(-1).contiguous()))
        shuffled = []
        for uu, ii in blocks:
            perm = torch.randperm(uu.numel(), generator=g, device="cuda")
            shuffled.append((uu[perm].contiguous(), ii[perm].contiguous()))

        def score():
            for uu, ii in blocks:
                e.score_pairs(uu, ii)

        r = {"case": "score_pairs", "dtype": dtype, "pairs": pairs, "block": a.block}
        r.update(windows(score))
        score_ms = r["ms"]
        print(json.dumps(r), flush=True)
        results.append(r)
        cases = [(top, maps, "grouped") for top in a.tops for maps in (False, True)] + [(a.tops[0], False, "shuffled")]
        for top, maps, order in cases:
            def explain():
                for uu, ii in (blocks if order == "grouped" else shuffled):
                    e.feat_explain(uu, ii, top=top, maps=maps)
            r = {"case": "feat_explain", "dtype": dtype, "top": top, "map": maps, "order": order, "pairs": pairs, "block": a.block}
            r.update(windows(explain))
            nbytes = pairs * D * esz + (pairs * D * 4 if maps else 0)
            r["bytes_bound_ms"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 3)
            r["fraction_of_bytes_bound"] = round(r["bytes_bound_ms"] / r["ms"], 3)
            r["ratio_to_score_pairs"] = round(r["ms"] / score_ms, 2)
            r["us_per_pair"] = round(r["ms"] * 1e3 / pairs, 4)
            print(json.dumps(r), flush=True)
            results.append(r)
        e.sync_check()
        e.close()
        del e
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
