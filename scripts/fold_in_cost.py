"""Cost of folding in users the model was not trained on (bprx_fold_in, bprx_score_rows_block, bprx_topk_lists) on the C2 shape
of DESIGN.md: I = 50 000, k = d = 64.

  fold_in          n = 100 000 new users x 20 positives x 4 negatives (80 pairs each), T = 30 steps, adam_tf23: ms per call = a timed
                   window of --reps calls / reps, the median of five windows with (min, max), for the default form (pair differences
                   kept in LDS where they fit) and for BPRX_FOLD_CACHE=0 (every step gathers the item rows again), each in an engine
                   of its own (the variable is read at create).  Beside it the bytes the T steps request: every pair of every step
                   asks for two rows of (k + d + 1) fp32 and its own two ids; the cached form asks LDS for the cached share of
                   them.  The binding roofline is the request rate of the cache level that holds the item tables (Gi + P: 29 MB,
                   L2 / Infinity Cache resident), quoted at the 8 TB/s HBM figure the project quotes everywhere as a LOWER bound of
                   that level: the fraction printed is therefore an upper bound of the true fraction.
  new-user block   score_rows_block + topk_lists for one block of --block folded rows, next to
  catalogue block  score_block + topk for as many trained users, in the same process.
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/fold_in_cost.py [--out profiles/fold_in_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402

U, I, K, DD, D = 4096, 50_000, 64, 64, 64
HBM_BYTES_PER_S = 8e12
TARGET = 0.5
LDS_SHARE_FLOATS = 2560                                             # bprx_foldin.hip: FOLD_SHARE


def windows(fn, reps, passes=5):
    fn()
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
    return {"ms": round(float(np.median(out)), 4), "ms_min_max": [round(min(out), 4), round(max(out), 4)], "calls_per_window": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--positives", type=int, default=20)
    ap.add_argument("--negatives", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3, help="fold_in calls per timed window")
    ap.add_argument("--block", type=int, default=4096, help="rows per score block")
    ap.add_argument("--block_reps", type=int, default=5)
    ap.add_argument("--top_k", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_in_cost.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, generator=g, device="cuda") * 2 - 1
    lim = lambda r, c: float(np.sqrt(6.0 / (r + c)))
    F = torch.rand((I, D), generator=g, device="cuda")
    t = dict(Gu=rnd(U, K) * lim(U, K), Gi=rnd(I, K) * lim(I, K), Bi=torch.zeros(I, device="cuda"), Tu=rnd(U, DD) * lim(U, DD),
             E=rnd(D, DD) * lim(D, DD), Bp=rnd(D) * lim(D, 1), F=F)
    n, npairs = a.users, a.positives * a.negatives
    ptr = torch.arange(n + 1, dtype=torch.int64, device="cuda") * npairs
    # (uniform items: the timing does not depend on a negative being outside the history)
    pos = torch.randint(I, (n, a.positives), generator=g, device="cuda", dtype=torch.int32).repeat_interleave(a.negatives, 1).reshape(-1)
    neg = torch.randint(I, (n * npairs,), generator=g, device="cuda", dtype=torch.int32)
    Gu, Tu = torch.zeros((n, K), device="cuda"), torch.zeros((n, DD), device="cuda")
    results = []
    row_bytes = 2 * (K + DD + 1) * 4 + 8
    epl = (K + DD + 63) // 64
    engines = {}
    for form, env in (("lds", None), ("regather", "0")):
        if env is None:
            os.environ.pop("BPRX_FOLD_CACHE", None)
        else:
            os.environ["BPRX_FOLD_CACHE"] = env
        e = Engine(model="vbpr", num_users=U, num_items=I, embed_k=K, embed_d=DD, feat_dim=D, feat_dtype="fp32", optimizer="adam_tf23",
                   lr=0.05, reg=1e-3, max_batch=4096).bind(**t)
        engines[form] = e

        def fold():
            Gu.zero_(); Tu.zero_()
            e.fold_in(ptr, pos, neg, a.steps, Gu, Tu, lr=0.05, reg=1e-3, optimizer="adam_tf23", want_loss=False)

        r = {"case": "fold_in", "form": form, "users": n, "pairs_per_user": npairs, "steps": a.steps, "optimizer": "adam_tf23",
             "items": I, "embed_k": K, "embed_d": DD}
        r.update(windows(fold, a.reps))
        fit = LDS_SHARE_FLOATS // (64 * epl + 1)
        cached = 0 if form == "regather" else (npairs if npairs <= fit else fit // 4 * 4)
        r["pairs_cached_in_lds"] = cached
        r["pair_evaluations"] = n * npairs * a.steps
        r["cache_bytes_requested"] = n * row_bytes * (cached + (npairs - cached) * a.steps)
        r["lds_bytes_requested"] = n * cached * a.steps * (64 * epl + 1) * 4
        r["bytes_bound_ms_at_8TBs"] = round(r["cache_bytes_requested"] / HBM_BYTES_PER_S * 1e3, 4)
        r["fraction_of_bytes_bound"] = round(r["bytes_bound_ms_at_8TBs"] / r["ms"], 3)
        r["reaches_design_target"] = bool(r["fraction_of_bytes_bound"] >= TARGET)
        r["pair_evaluations_per_us"] = round(r["pair_evaluations"] / (r["ms"] * 1e3), 1)
        print(json.dumps(r), flush=True)
        results.append(r)
    os.environ.pop("BPRX_FOLD_CACHE", None)
    results[0]["ratio_to_regather"] = round(results[0]["ms"] / results[1]["ms"], 3)
    results[0]["next"] = ("the share of LDS per wave is what four workgroups per CU leave (40 KB per workgroup, "
                          "profiles/fold_in_share_sweep.jsonl); the pairs of a long history beyond it are gathered again every step, and "
                          "a group's chain dot -> wave_sum -> exp -> axpy is latency-bound at four waves per SIMD.  At k + d <= 128 a "
                          "HALF-wave per user (four elements per lane, a five-level reduction) would double the users in flight on "
                          "the same registers and LDS")

    e = engines["lds"]
    nu = min(a.block, U, n)
    hist = torch.randint(I, (nu, a.positives), generator=g, device="cuda", dtype=torch.int32)
    lists = (torch.arange(nu + 1, dtype=torch.int64, device="cuda") * a.positives, hist.reshape(-1).contiguous())
    csr = (torch.cat([lists[0], lists[0][-1:].expand(U - nu)]), lists[1])
    out_new = torch.empty((nu, I), dtype=torch.float32, device="cuda")
    out_cat = torch.empty((nu, I), dtype=torch.float32, device="cuda")

    def new_block():
        e.topk_lists(e.score_rows_block(Gu, Tu, 0, nu, out=out_new), lists, a.top_k)

    def cat_block():
        e.topk(0, nu, e.score_block(0, nu, out=out_cat), csr, a.top_k)

    for case, fn in (("new_user_block", new_block), ("catalogue_block", cat_block)):
        r = {"case": case, "rows": nu, "items": I, "top_k": a.top_k}
        r.update(windows(fn, a.block_reps))
        print(json.dumps(r), flush=True)
        results.append(r)
    results[-2]["ratio_to_catalogue_block"] = round(results[-2]["ms"] / results[-1]["ms"], 3)
    for e in engines.values():
        e.sync_check()
        e.close()
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
