"""Cost of calibrated lists for every user (bprx_calibrate behind bprx_score_block + bprx_topk) on the C2 shape of DESIGN.md:
U = 100 000 users, I = 50 000 items, k = d = 64, D = 4 096, bf16 features, K = 20 per list picked from a pool of N = 100, class
tables of C = 64 and C = 1 024 classes (uniform), 20 history items per user, lambda = 0.5, alpha = 0.01.  Device work only: the
download of the lists and their upload as pools (ranking.calibrate_rows) are the host's.

Each timing is the median of five windows with (min, max), all in one process, from device events around whole calls that end in
a synchronise; the windows of the cases alternate (case A, case B, ..., five times over), so that drift hits every case alike:

  plain             every user block's bprx_score_block + bprx_topk with K = 20: what recs-* costs today
  pool_calibrate    every user block's bprx_score_block + bprx_topk with K = N, then bprx_calibrate on the block's pools, per C
  calibrate         bprx_calibrate alone over the pools of ALL users, per C
  diversify         bprx_diversify alone over the same pools (theta = 0.5; latent, w = 64, and both, w = 128)

`summary` holds the share of the plain pass and the ratio to bprx_diversify with their spread (from the windows' min / max).

quality: the clustered synth (synth.make_interactions_clustered, 20 groups) with the groups as the classes, BPRMF trained for 400
steps: mean kl_plain against mean kl_calibrated and the test HR@20 of the calibrated lists against the plain ones, lambda = 0.5
and 0.9.
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/calibrate_cost.py [--out profiles/calibrate_cost.json] [--skip quality]"""
import argparse
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd import synth  # noqa: E402
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402

U, I, K, DD, D = 100_000, 50_000, 64, 64, 4096


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def cost(a, results):
    nu, n, Df, topk, N, H = a.users, a.items, a.feat_dim, a.top_k, a.pool, a.history
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
    tables = {C: torch.randint(0, C, (n,), generator=g, device="cuda", dtype=torch.int32) for C in a.classes}
    blocks = [(u0, min(nu, u0 + a.block)) for u0 in range(0, nu, a.block)]
    scores = torch.empty((a.block, n), dtype=torch.float32, device="cuda")
    pi = torch.empty((nu, N), dtype=torch.int32, device="cuda")
    pv = torch.empty((nu, N), dtype=torch.float32, device="cuda")

    def ranked(kq, C=None, keep=False):
        for u0, u1 in blocks:
            idx, val, _ = e.topk(u0, u1, e.score_block(u0, u1, out=scores[:u1 - u0]), train, kq)
            if keep:
                pi[u0:u1], pv[u0:u1] = idx, val
            if C is not None:
                e.calibrate(idx, val, train, tables[C], C, topk, a.lam, a.alpha, row0=u0)

    ranked(N, keep=True)                                            # the pools of all users, once
    rn = {space: e.sim_rnorm(space) for space in a.spaces}
    width = {"latent": K, "visual": DD, "both": K + DD}
    cases = [("plain", lambda: ranked(topk), {"users": nu, "items": n, "top_k": topk, "blocks": len(blocks)})]
    for C in a.classes:
        cases.append(("pool_calibrate C=%d" % C, lambda C=C: ranked(N, C),
                      {"users": nu, "items": n, "pool": N, "top_k": topk, "classes": C, "lambda": a.lam, "alpha": a.alpha}))
    for C in a.classes:
        cases.append(("calibrate C=%d" % C, lambda C=C: e.calibrate(pi, pv, train, tables[C], C, topk, a.lam, a.alpha),
                      {"users": nu, "pool": N, "top_k": topk, "classes": C, "history": H, "lambda": a.lam, "alpha": a.alpha,
                       "lds_bytes_per_list": 12 * C + 208}))
    for space in a.spaces:
        cases.append(("diversify %s" % space, lambda s=space: e.diversify(s, rn[s], pi, pv, topk, 0.5),
                      {"users": nu, "pool": N, "top_k": topk, "space": space, "width": width[space], "theta": 0.5}))
    reps, times = {}, {name: [] for name, _, _ in cases}
    for name, fn, _ in cases:                                        # warm-up: code objects, the allocator's blocks, clocks
        fn()
        torch.cuda.synchronize()
        reps[name] = max(1, int(np.ceil(a.window_ms / max(timed(fn, 1), 1e-3))))
    for _ in range(5):
        for name, fn, _ in cases:
            times[name].append(timed(fn, reps[name]))
    rows = {}
    for name, _, info in cases:
        ts = times[name]
        r = {"case": name, **info, "ms": round(float(np.median(ts)), 4), "ms_min_max": [round(min(ts), 4), round(max(ts), 4)],
             "passes_per_window": reps[name]}
        rows[name] = r
        print(json.dumps(r), flush=True)
        results.append(r)
    ratio = lambda x, y: {"median": round(rows[x]["ms"] / rows[y]["ms"], 4),
                          "min_max": [round(rows[x]["ms_min_max"][0] / rows[y]["ms_min_max"][1], 4),
                                      round(rows[x]["ms_min_max"][1] / rows[y]["ms_min_max"][0], 4)]}
    s = {"case": "summary"}
    for C in a.classes:
        s["calibrate C=%d share of plain" % C] = ratio("calibrate C=%d" % C, "plain")
        s["pool_calibrate C=%d times plain" % C] = ratio("pool_calibrate C=%d" % C, "plain")
        for space in a.spaces:
            s["calibrate C=%d over diversify %s" % (C, space)] = ratio("calibrate C=%d" % C, "diversify %s" % space)
    print(json.dumps(s), flush=True)
    results.append(s)
    e.sync_check()
    e.close()


def quality(a, results):
    from fashionvisualexpl_recommend_amd.models import BPRMF
    from fashionvisualexpl_recommend_amd.ranking import rank_rows
    nu, n, G, seed = 2000, 3000, 20, 1
    tr, va, te = synth.make_interactions_clustered(nu, n, per_user=22, clusters=G, seed=seed)
    cluster = np.random.RandomState(seed).randint(G, size=n)        # make_interactions_clustered's first draw
    p = Namespace(dataset="synth", validation=True, batch_size=4096, epochs=1, batch_eval=4096, embed_k=32, embed_d=0, lr=0.05,
                  reg=1e-3, top_k=a.top_k, verbose=-1, restore_epochs=1, rec="bprmf", best_metric="ndcg", optimizer="sgd", init_seed=0,
                  dtype="bf16", calibrate_pool=a.pool)
    data = Namespace(training_list=tr, validation_list=va, test_list=te, num_users=nu, num_items=n, params=p)
    m = BPRMF(data, p)
    rs = np.random.RandomState(2)
    users = np.repeat(np.arange(nu), [len(l) for l in tr]).astype(np.int32)
    pos = np.concatenate([np.asarray(l) for l in tr]).astype(np.int32)
    steps, B = 400, 4096
    for _ in range(steps):
        pick = rs.randint(users.size, size=B)
        neg = rs.randint(n, size=B).astype(np.int32)
        m.engine.step(*(torch.as_tensor(x, device="cuda") for x in (users[pick], pos[pick], neg)))
    test = np.array([l[0] for l in te])
    hr = lambda ids: round(float((ids == test[:, None]).any(1).mean()), 4)
    m.evaluator._metrics_device_csr()
    plain, _, _ = rank_rows(m.evaluator._topk(0, nu), m.engine.score_block(0, nu), a.top_k)
    for lam in (0.5, 0.9):
        ids, vals, cls, gain, kl = m.recommend_calibrated(lam=lam, alpha=a.alpha, classes=cluster)
        r = {"case": "quality", "users": nu, "items": n, "groups": G, "classes": G, "train_steps": steps, "top_k": a.top_k, "pool": a.pool,
             "lambda": lam, "alpha": a.alpha, "kl_plain_mean": round(float(kl[:, 0].mean()), 5),
             "kl_calibrated_mean": round(float(kl[:, 1].mean()), 5), "hr_plain": hr(plain), "hr_calibrated": hr(ids),
             "lists_changed": round(float((ids != plain).any(1).mean()), 4)}
        print(json.dumps(r), flush=True)
        results.append(r)
    m.engine.sync_check()
    m.engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=U, help="users (a rehearsal takes fewer)")
    ap.add_argument("--items", type=int, default=I)
    ap.add_argument("--feat_dim", type=int, default=D)
    ap.add_argument("--top_k", type=int, default=20)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--classes", nargs="+", type=int, default=[64, 1024])
    ap.add_argument("--history", type=int, default=20, help="history items per user")
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--spaces", nargs="+", default=["latent", "both"])
    ap.add_argument("--block", type=int, default=4096, help="users per score block (Evaluator.user_block)")
    ap.add_argument("--window_ms", type=float, default=200.0)
    ap.add_argument("--skip", nargs="*", default=[], choices=["cost", "quality"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate_cost.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    results = []
    if "cost" not in a.skip:
        cost(a, results)
    if "quality" not in a.skip:
        quality(a, results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
