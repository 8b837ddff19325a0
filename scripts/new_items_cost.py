"""Cost of scoring items the model was not trained on (bprx_project_rows, bprx_score_new_block, bprx_topk_rows) on the C2 shape of
DESIGN.md: U = 100 000, k = d = 64, D = 4 096, bf16 features, n = 50 000 new rows (as many as the catalogue holds).

  project_rows     one pass over the n x D bf16 table.  ms per call = a timed window of --reps calls / reps, the median of five
                   windows with (min, max).  Beside it the bytes bound n D 2 / 8 TB/s, the achieved fraction of it, and the time
                   of the catalogue's own forward projection of as many rows (k_proj_fwd_bf16_v10, the mean of the kernel trace in
                   profiles/r03_bench_c2_kernel_stats.csv when that file is there).
  new block        score_new_block + topk_rows for one block of --block users against n new items, next to
  catalogue block  score_block + topk for the same users against the I = n catalogue items, in the same process (windows of
                   --block_reps blocks).
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/new_items_cost.py [--out profiles/new_items_cost.json]"""
import argparse
import csv
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
TARGET = 0.5                                                        # the project's design target: share of the binding roofline


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
    return {"ms": round(float(np.median(out)), 4), "ms_min_max": [round(min(out), 4), round(max(out), 4)], "calls_per_window": reps}


def catalogue_kernel_us():
    """Mean time of k_proj_fwd_bf16_v10 in the recorded C2 kernel trace (ns -> us), or None."""
    path = os.path.join(ROOT, "profiles", "r03_bench_c2_kernel_stats.csv")
    if not os.path.exists(path):
        return None
    for row in csv.reader(open(path)):
        if row and "k_proj_fwd_bf16_v10" in row[0]:
            return round(float(row[3]) / 1e3, 2)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=I, help="new rows (a rehearsal takes fewer)")
    ap.add_argument("--block", type=int, default=4096, help="users per score block")
    ap.add_argument("--reps", type=int, default=200, help="project_rows calls per timed window")
    ap.add_argument("--block_reps", type=int, default=5, help="user blocks per timed window")
    ap.add_argument("--top_k", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_items_cost.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, generator=g, device="cuda") * 2 - 1
    lim = lambda r, c: float(np.sqrt(6.0 / (r + c)))
    t = dict(Gu=rnd(U, K) * lim(U, K), Gi=rnd(I, K) * lim(I, K), Bi=torch.zeros(I, device="cuda"), Tu=rnd(U, DD) * lim(U, DD),
             E=rnd(D, DD) * lim(D, DD), Bp=rnd(D) * lim(D, 1))

    def table(rows):
        F = torch.randn((rows, D), generator=g, device="cuda").abs_()
        F *= torch.rand((rows, D), generator=g, device="cuda") < 0.5  # relu-like: about half zeros
        return (F / F.max()).to(torch.bfloat16)

    e = Engine(model="vbpr", num_users=U, num_items=I, embed_k=K, embed_d=DD, feat_dim=D, feat_dtype="bf16", optimizer="sgd",
               lr=0.05, reg=0.0, max_batch=4096).bind(**t, F=table(I))
    n = a.rows
    Fnew = table(n)
    results = []

    r = {"case": "project_rows", "dtype": "bf16", "rows": n, "feat_dim": D, "embed_d": DD}
    r.update(windows(lambda: e.project_rows(Fnew), a.reps))
    r["bytes_bound_ms"] = round(n * D * 2 / HBM_BYTES_PER_S * 1e3, 4)
    r["fraction_of_bytes_bound"] = round(r["bytes_bound_ms"] / r["ms"], 3)
    r["reaches_design_target"] = bool(r["fraction_of_bytes_bound"] >= TARGET)
    cat = catalogue_kernel_us()
    if cat is not None:
        r["catalogue_k_proj_fwd_bf16_v10_us_for_50000_rows"] = cat
        r["ratio_to_catalogue_kernel_per_row"] = round((r["ms"] * 1e3 / n) / (cat / 50_000), 3)
    print(json.dumps(r), flush=True)
    results.append(r)

    P = e.project_rows(Fnew)
    nu = min(a.block, U)
    csr = (torch.zeros(U + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))   # nothing masked
    out_new = torch.empty((nu, n), dtype=torch.float32, device="cuda")
    out_cat = torch.empty((nu, I), dtype=torch.float32, device="cuda")

    def new_block():
        e.topk_rows(e.score_new_block(0, nu, P, out=out_new), a.top_k)

    def cat_block():
        e.topk(0, nu, e.score_block(0, nu, out=out_cat), csr, a.top_k)

    e.score_block(0, nu, out=out_cat)                               # (the catalogue's own projection: once per parameter state)
    for case, fn, width in (("new_block", new_block, n), ("catalogue_block", cat_block, I)):
        r = {"case": case, "users": nu, "items": width, "top_k": a.top_k}
        r.update(windows(fn, a.block_reps))
        print(json.dumps(r), flush=True)
        results.append(r)
    results[-2]["ratio_to_catalogue_block"] = round(results[-2]["ms"] / results[-1]["ms"], 3)
    print(json.dumps(results[-2]), flush=True)
    e.sync_check()
    e.close()
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
