"""Cost of hard negatives (bprx_sample_*_hard, bprx_hard_snapshot) on the C2 shape of DESIGN.md: U = 100 000 users, I = 50 000
items, k = d = 64, D = 4 096, bf16 features, B = 65 536 triplets per batch, 20 positives per user, the epoch walk.

Device-event times, all versions ALTERNATING in one process (five windows each, median with (min, max)):

  sample          the uniform sampler (C = 1 of the hard one is the same stream) and the hard one at C = 2, 4, 8
  sample + step   the same, each followed by the step it feeds
  refresh         one snapshot of the item projections (the forward projection of every item into the sampler's buffer)

Beside every hard `sample`: the bytes of the rows the kernel gathers -- B (C (4 k + 4 (d + 1) + 4) + 4 (k + d)) -- over its time
minus the uniform sampler's (the draw of candidate 0 and the writes are common to both), next to the estimate of the issue
(C = 8: ~280 MB of candidate rows + 33 MB of user rows, "several tens of us").
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/hard_negatives_cost.py [--out profiles/hard_negatives_cost.json] [--kernel_only]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd.engine import Engine, EpochWalkSampler  # noqa: E402

U, I, K, DD, D, B, NPU = 100_000, 50_000, 64, 64, 4096, 65_536, 20


def alternate(fns, reps, passes=5):
    """{name: {"ms", "ms_min_max"}}: per pass one window of `reps` calls of every version, in turn."""
    for fn in fns.values():
        fn()                                                        # warm-up: code objects, the allocator's blocks, clocks
    torch.cuda.synchronize()
    got = {n: [] for n in fns}
    for _ in range(passes):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            got[n].append(a.elapsed_time(b) / reps)
    return {n: {"ms": round(float(np.median(v)), 5), "ms_min_max": [round(min(v), 5), round(max(v), 5)], "calls_per_window": reps}
            for n, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=U, help="users (a rehearsal takes fewer)")
    ap.add_argument("--items", type=int, default=I)
    ap.add_argument("--feat_dim", type=int, default=D)
    ap.add_argument("--batch", type=int, default=B)
    ap.add_argument("--candidates", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--kernel_only", action="store_true", help="a few hard samples and nothing else: the run a kernel trace wraps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hard_negatives_cost.json"))
    a = ap.parse_args()
    nu, n, Df, nb = a.users, a.items, a.feat_dim, a.batch
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
               lr=0.05, reg=0.0, max_batch=nb).bind(**t)
    items = torch.randint(n, (nu, NPU), generator=g, device="cuda", dtype=torch.int32).sort(dim=1).values.reshape(-1)
    indptr = torch.arange(nu + 1, device="cuda", dtype=torch.int64) * NPU
    pos_user = torch.arange(nu, device="cuda", dtype=torch.int32).repeat_interleave(NPU)
    new = lambda: EpochWalkSampler.from_csr(indptr, items, pos_user, n, seed=2024)
    out = tuple(torch.empty(nb, dtype=torch.int32, device="cuda") for _ in range(3))
    samplers = {"uniform": new().feeds(e)}
    samplers.update({"hard_C%d" % c: new().hard(e, c) for c in a.candidates})
    if a.kernel_only:
        for s in samplers.values():
            for _ in range(10):
                s.sample(nb, out=out)
        torch.cuda.synchronize()
        e.sync_check()
        return
    results = []
    shape = {"users": nu, "items": n, "k": K, "d": DD, "feat_dim": Df, "batch": nb, "sampler": "epoch walk", "features": "bf16"}
    res = alternate({name: (lambda s=s: s.sample(nb, out=out)) for name, s in samplers.items()}, 20)
    base = res["uniform"]["ms"]
    for name, r in res.items():
        r = dict(case="sample", version=name, **shape, **r)
        if name != "uniform":
            c = int(name.split("C")[1])
            gathered = nb * (c * (4 * K + 4 * (DD + 1) + 4) + 4 * (K + DD))
            r.update(candidates=c, gathered_row_bytes=gathered, over_uniform_ms=round(r["ms"] - base, 5),
                     gathered_TB_per_s_over_whole_kernel=round(gathered / (r["ms"] * 1e-3) / 1e12, 3))
        print(json.dumps(r), flush=True)
        results.append(r)

    def with_step(s):
        e.step(*s.sample(nb, out=out), want_loss=False)
    res = alternate({name: (lambda s=s: with_step(s)) for name, s in samplers.items()}, 10)
    for name, r in res.items():
        r = dict(case="sample+step", version=name, **shape, **r)
        print(json.dumps(r), flush=True)
        results.append(r)
    e.settle()
    hard = samplers["hard_C%d" % a.candidates[0]]
    r = dict(case="refresh", **shape, **alternate({"refresh": hard.refresh}, 5)["refresh"])
    r["snapshot_bytes"] = int(hard.snapshot.numel() * 4)
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
