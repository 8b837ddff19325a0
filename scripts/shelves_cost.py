"""Cost of category shelves (bprx_score_block + bprx_topk_classes) for one block of users on the C2 shape of DESIGN.md: a block of
4 096 users against I = 50 000 items, k = d = 64, D = 4 096, bf16 features, K = 20 per list, 20 training items per user.  Two class
tables, C = 16 and C = 256, both with Zipf-distributed sizes (class c holds about I / ((c + 1) H_C) items, the smallest at least
one), the items of a class scattered over the catalogue.

Per class table three passes over the same block, all in one process:

  plain       bprx_score_block + bprx_topk with K = 20: the plain ranking pass, what recs-* costs today
  shelves     bprx_score_block + bprx_topk_classes with K = 20
  torch       the composition one could write without the kernel: bprx_score_block, the training items masked by index_put_,
              index_select of the block into class order, then torch.topk per class slice (k = min(20, class size))
  *_ranking   the ranking half alone on a block of scores that is already there

Each timing is the median of five windows with (min, max) from device events around work that ends in a synchronise; a window
repeats its pass until it lasts about 0.3 s, and the windows of the cases alternate (case A, case B, ..., five times over), so
that drift hits every case alike.  Device work only: the download of the lists is the host's.

Prints one JSON line per case and writes them all to --out.
Usage: python scripts/shelves_cost.py [--out profiles/shelves_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402
from fashionvisualexpl_recommend_amd.ranking import class_csr  # noqa: E402

I, K, DD, D = 50_000, 64, 64, 4096


def zipf_classes(n, C, seed):
    """The class of every item: sizes ~ 1 / rank over C classes, every class at least one item, items assigned at random."""
    w = 1.0 / np.arange(1, C + 1)
    sizes = np.maximum(1, np.floor(w / w.sum() * n).astype(np.int64))
    sizes[0] += n - sizes.sum()
    assert sizes.min() >= 1 and sizes.sum() == n
    return np.repeat(np.arange(C), sizes)[np.random.RandomState(seed).permutation(n)], sizes


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=4096, help="users of the block (a rehearsal takes fewer)")
    ap.add_argument("--items", type=int, default=I)
    ap.add_argument("--feat_dim", type=int, default=D)
    ap.add_argument("--top_k", type=int, default=20)
    ap.add_argument("--history", type=int, default=20, help="training items per user")
    ap.add_argument("--classes", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--window_ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shelves_cost.json"))
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
    mask_rows, mask_cols = torch.arange(nu, device="cuda").repeat_interleave(H), items.long()
    buf = torch.empty((nu, n), dtype=torch.float32, device="cuda")
    ninf = torch.tensor(float("-inf"), device="cuda")
    e.score_block(0, 1)                                              # (P is made current here, once per parameter state)
    cases = []

    def plain():
        e.topk(0, nu, e.score_block(0, nu, out=buf), train, topk)

    cases.append(("plain", plain, {}))
    cases.append(("plain_ranking", lambda: e.topk(0, nu, buf, train, topk), {}))     # (the block is masked already: the same work)
    for C in a.classes:
        cls, sizes = zipf_classes(n, C, seed=C)
        ccsr = class_csr(cls, n, "cuda")
        order, cuts = ccsr[1].long(), ccsr[0].cpu().tolist()
        info = {"classes": C, "largest_class": int(sizes.max()), "smallest_class": int(sizes.min())}

        def shelves_ranking(ccsr=ccsr):
            e.topk_classes(buf, train, ccsr, topk)

        def shelves(ccsr=ccsr):
            e.topk_classes(e.score_block(0, nu, out=buf), train, ccsr, topk)

        def torch_ranking(order=order, cuts=cuts):
            buf.index_put_((mask_rows, mask_cols), ninf)
            by_class = buf.index_select(1, order)
            return [torch.topk(by_class[:, cuts[c]:cuts[c + 1]], min(topk, cuts[c + 1] - cuts[c]), dim=1) for c in range(len(cuts) - 1)]

        def torch_pass(rank=torch_ranking):
            e.score_block(0, nu, out=buf)
            rank()

        cases += [("shelves_C%d" % C, shelves, info), ("torch_C%d" % C, torch_pass, info),
                  ("shelves_ranking_C%d" % C, shelves_ranking, info), ("torch_ranking_C%d" % C, torch_ranking, info)]
    reps, times = {}, {name: [] for name, _, _ in cases}
    for name, fn, _ in cases:                                        # warm-up: code objects, the allocator's blocks, clocks
        fn()
        torch.cuda.synchronize()
        reps[name] = max(1, int(np.ceil(a.window_ms / max(timed(fn, 1), 1e-3))))
    for _ in range(5):
        for name, fn, _ in cases:
            times[name].append(timed(fn, reps[name]))
    e.sync_check()
    e.close()
    results = []
    for name, _, info in cases:
        ts = times[name]
        r = {"case": name, "users": nu, "items": n, "top_k": topk, "history": H}
        r.update(info)
        r.update({"ms": round(float(np.median(ts)), 4), "ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "passes_per_window": reps[name]})
        r["ratio_to_plain"] = round(r["ms"] / float(np.median(times["plain"])), 4)
        print(json.dumps(r), flush=True)
        results.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
