"""Cost of the style clusters (bprx_style_assign / bprx_style_update, models.item_styles' loop) on the C2 catalogue of DESIGN.md:
I = 50 000 items, k = d = 64, D = 4 096, bf16 features, the visual space (w = 64), S = 64 and S = 1024 styles.

  assign_S     one bprx_style_assign pass over the whole catalogue against S centroids
  update_S     one bprx_style_update pass over the S clusters of that assignment
  loop_S       the whole clustering as models.item_styles runs it at T = 20: farthest-first seeds, then per iteration the update,
               the assignment and the host's CSR of it, until nothing changes or 20 iterations have run (wall time; the
               iterations run are recorded)
  plain        bprx_score_block + bprx_topk (K = 20) for a block of 4 096 users: one block of the plain ranking pass behind recs-*

Each kernel timing is the median of five windows with (min, max) from device events; a window repeats its pass until it lasts
about 0.2 s, and the windows of the cases alternate.  The loop is timed by the host clock around a synchronise, three times.
The floor of an assignment pass is max(table bytes / HBM peak, 2 I S w / fp32-MFMA peak) with 8 TB/s and 155 TF.

`clustered` trains BPRMF (k = 32) on synth.make_interactions_clustered (2 000 users, 3 000 items, 20 groups) for a few hundred steps
and clusters its latent space with S = 20: the iterations to convergence and the final objective are recorded.

Prints one JSON line per case and writes them all to --out.
Usage: python scripts/styles_cost.py [--out profiles/styles_cost.json]"""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd import synth  # noqa: E402
from fashionvisualexpl_recommend_amd.models import BPRMF, VBPR  # noqa: E402
from fashionvisualexpl_recommend_amd.ranking import class_csr  # noqa: E402

HBM_PEAK, MFMA_FP32_PEAK = 8.0e12, 155.0e12


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def params(rec, k, d, **kw):
    return Namespace(dataset="synth", validation=True, batch_size=4096, epochs=1, batch_eval=4096, embed_k=k, embed_d=d, lr=0.05,
                     reg=1e-3, top_k=20, verbose=-1, restore_epochs=1, rec=rec, best_metric="ndcg", optimizer="sgd", init_seed=0,
                     dtype="bf16", **kw)


def clustered(out):
    U, I, G = 2000, 3000, 20
    tr, va, te = synth.make_interactions_clustered(U, I, per_user=22, clusters=G, seed=1)
    data = Namespace(training_list=tr, validation_list=va, test_list=te, num_users=U, num_items=I, params=params("bprmf", 32, 0))
    m = BPRMF(data, params("bprmf", 32, 0, styles=G))
    rs = np.random.RandomState(2)
    users = np.repeat(np.arange(U), [len(l) for l in tr]).astype(np.int32)
    pos = np.concatenate([np.asarray(l) for l in tr]).astype(np.int32)
    steps, B = 400, 4096
    for _ in range(steps):
        pick = rs.randint(users.size, size=B)
        neg = rs.randint(I, size=B).astype(np.int32)
        m.engine.step(*(torch.as_tensor(x, device="cuda") for x in (users[pick], pos[pick], neg)))
    style, cos, cent, obj = m.item_styles()
    m.engine.close()
    r = {"case": "clustered", "users": U, "items": I, "groups": G, "styles": G, "space": "latent", "width": 32, "train_steps": steps,
         "iterations": int(obj.size), "objective_first": round(float(obj[0]), 6), "objective_final": round(float(obj[-1]), 6),
         "largest_style": int(np.bincount(style[style >= 0], minlength=G).max()),
         "smallest_style": int(np.bincount(style[style >= 0], minlength=G).min())}
    print(json.dumps(r), flush=True)
    out.append(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=50_000)
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--feat_dim", type=int, default=4096)
    ap.add_argument("--styles", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--window_ms", type=float, default=200.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "styles_cost.json"))
    a = ap.parse_args()
    I, U, D, k, d = a.items, a.users, a.feat_dim, 64, 64
    torch.cuda.set_device(0)
    results = []
    tr, va, te = synth.make_interactions(U, I, per_user=20, seed=3)
    data = Namespace(training_list=tr, validation_list=va, test_list=te, num_users=U, num_items=I, params=params("vbpr", k, d))
    m = VBPR(data, params("vbpr", k, d), features=synth.make_features(I, D, seed=4))
    e = m.engine
    rn = e.sim_rnorm("visual")
    train = e.csr([list(l) for l in tr])
    buf = torch.empty((U, I), dtype=torch.float32, device="cuda")
    cases = [("plain", lambda: e.topk(0, U, e.score_block(0, U, out=buf), train, 20), {"users": U, "top_k": 20})]
    loops = {}
    for S in a.styles:
        t0 = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            style, cos, cent, obj = m.item_styles(S=S, iters=20, space="visual")
            torch.cuda.synchronize()
            t0.append((time.perf_counter() - t) * 1e3)
        t1 = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            m.style_seeds(S, "visual")
            torch.cuda.synchronize()
            t1.append((time.perf_counter() - t) * 1e3)
        loops[S] = {"ms": round(float(np.median(t0)), 3), "ms_min_max": [round(min(t0), 3), round(max(t0), 3)],
                    "seeds_ms": round(float(np.median(t1)), 3), "iterations": int(obj.size), "objective_final": round(float(obj[-1]), 6)}
        ct = torch.as_tensor(cent, device="cuda")
        csr = class_csr(style, I, "cuda", classes=S)
        floor = max((I * e.proj_stride() * 4 + S * d * 4 + I * 12) / HBM_PEAK, 2.0 * I * S * d / MFMA_FP32_PEAK) * 1e3
        cases.append(("assign_S%d" % S, lambda ct=ct: e.style_assign("visual", ct, 0, I, rn, want_second=False),
                      {"styles": S, "floor_ms": round(floor, 5)}))
        cases.append(("update_S%d" % S, lambda ct=ct, csr=csr: e.style_update("visual", rn, csr, ct),
                      {"styles": S, "floor_ms": round((I * e.proj_stride() * 4) / HBM_PEAK * 1e3, 5),
                       "largest_style": int(np.bincount(style, minlength=S).max())}))
    reps, times = {}, {name: [] for name, _, _ in cases}
    for name, fn, _ in cases:
        fn()
        torch.cuda.synchronize()
        reps[name] = max(1, int(np.ceil(a.window_ms / max(timed(fn, 1), 1e-3))))
    for _ in range(5):
        for name, fn, _ in cases:
            times[name].append(timed(fn, reps[name]))
    e.sync_check()
    plain = float(np.median(times["plain"]))
    for name, _, info in cases:
        ts = times[name]
        r = {"case": name, "items": I, "space": "visual", "width": d}
        r.update(info)
        r.update({"ms": round(float(np.median(ts)), 4), "ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "passes_per_window": reps[name]})
        if "floor_ms" in r:
            r["ratio_to_floor"] = round(r["ms"] / r["floor_ms"], 2)
        print(json.dumps(r), flush=True)
        results.append(r)
    for S, r in loops.items():
        r = dict({"case": "loop_S%d" % S, "items": I, "space": "visual", "width": d, "styles": S, "max_iters": 20}, **r)
        r["ratio_to_plain_block"] = round(r["ms"] / plain, 2)
        print(json.dumps(r), flush=True)
        results.append(r)
    e.close()
    clustered(results)
    results.append({"case": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip})
    print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
