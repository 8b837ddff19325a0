"""Cost and quality of warm items and audiences for AttentiveFashion (bprx_af_fold_in_items, bprx_af_audience_block) at the
model's default k = 128, h = 64.

cost     n = 1 024 new items with 8, 40 and 320 pairs each (roles alternate), T = 30 steps, adam_tf23, 20 000 users, 2 048
         catalogue items: ms per call = a timed window of --reps calls / reps, the median of five windows with (min, max):
           af_fold_in_items    the whole call; pair forming and the fit apart: a call with T = 1 against the call with T = 30
                               (fit_ms = (ms_T - ms_1) T / (T - 1), pairs_ms = ms_T - fit_ms; the catalogue encodings are current)
           torch               batched torch-GPU autograd of the same loss: pair terms formed once by batched attention forwards,
                               then T steps of autograd and the same sparse-rule Adam on a [n, k] leaf
           fold_in_items       bprx_fold_in_items on a BPRMF handle of the same k and pair counts
blocks   bprx_af_audience_block (the catalogue form) against bprx_af_score_block over the same number of (user, item) pairs, scores
         and attentions: what the transposed store costs.
quality  clustered synth (synth.make_interactions_clustered), inputs that carry the item's cluster (edge image: the cluster's stroke
         pattern + noise; histogram: prototype + noise; class: the cluster one-hot for 70 % of the items).  AttentiveFashion is trained
         without a held-out tenth of the items; each held-out item is fitted from m = 2, 5, 20 of its buyers (zero start rows,
         adam_tf23) and its audience ranked with those buyers masked: HR@20 of the remaining buyers, one at a time, next to the same
         items trained IN the catalogue with the interactions of exactly those m buyers.
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/af_item_fold_cost.py [--out profiles/af_item_fold_cost.json] [--skip quality]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd import _ffi, synth  # noqa: E402
from fashionvisualexpl_recommend_amd.engine import Engine, PhiloxSampler  # noqa: E402
from fashionvisualexpl_recommend_amd.models import draw_item_fold_pairs  # noqa: E402

K, H, DC, DK = 128, 64, 64, 16
LR, REG, B1, B2, EPS = 0.05, 1e-3, 0.9, 0.999, 1e-7
ATT = ("attention.W_1", "attention.b_1", "attention.W_2", "attention.b_2")


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


def af_tables(rs, U, I, k=K, h=H):
    g = synth.glorot_uniform
    lim = np.sqrt(6.0 / (25 + 25 * 64))
    z = lambda n: np.zeros(n, np.float32)
    return {"Gu": g(rs, U, k), "Gi": g(rs, I, k), "Bi": z(I),
            "color.W1": g(rs, DC, 256), "color.b1": z(256), "color.W2": g(rs, 256, k),
            "edges.conv": rs.uniform(-lim, lim, size=(25, 64)).astype(np.float32), "edges.conv_b": z(64), "edges.W2": g(rs, 64, k),
            "class.W1": g(rs, DK, 256), "class.b1": z(256), "class.W2": g(rs, 256, k),
            "attention.W_1": g(rs, k, h), "attention.b_1": z(h), "attention.W_2": g(rs, h, 1), "attention.b_2": z(1)}


def af_engine(t, inputs, U, I, optimizer="adam_tf23", lr=LR, reg=REG, B=1024, k=K, rate=0.5):
    e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=k, optimizer=optimizer, lr=lr, reg=reg, max_batch=B)
    return e.bind_attentive(t["Gu"], t["Gi"], t["Bi"], *inputs, {n: t[n] for n in _ffi.AF_WEIGHTS}, dropout=rate, seed=0)


def random_inputs(rs, n):
    ed = (rs.random_sample((n, 28, 28)) < 0.15).astype(np.uint8).repeat(8, 1).repeat(8, 2) * np.uint8(200)
    col = rs.random_sample((n, DC)).astype(np.float32)
    cl = np.zeros((n, DK), np.float32)
    cl[np.arange(n), rs.randint(DK, size=n)] = 1.0
    return ed, col / np.abs(col).max(1, keepdims=True), cl


def att_alpha(gu, c, t):
    """alpha [..., 3] of rows gu [..., k] against encodings c [..., 3, k] (torch)."""
    a = torch.relu((gu.unsqueeze(-2) * c) @ t[ATT[0]] + t[ATT[1]]) @ t[ATT[2]].reshape(-1) + t[ATT[3]].reshape(())
    return torch.softmax(a, -1)


def torch_fold(t, Call, Cn, user, other, role, n, npairs, steps):
    """The definition of include/bprx.h with autograd, all items in one batch; returns W [n, k]."""
    u, o = user.long().view(n, npairs), other.long().view(n, npairs)
    s = 1.0 - 2.0 * role.float().view(n, npairs)
    gu = t["Gu"][u]                                                   # [n, np, k]
    cr = Cn.permute(1, 0, 2)[:, None].expand(-1, npairs, -1, -1)      # [n, np, 3, k]
    m = gu * (att_alpha(gu, cr, t).unsqueeze(-1) * cr).sum(-2)
    co = Call.permute(1, 0, 2)[o]                                     # [n, np, 3, k]
    xo = (att_alpha(gu, co, t) * (co * (gu * t["Gi"][o]).unsqueeze(-2)).sum(-1)).sum(-1)
    Dm, dc = s[:, :, None] * m, -s * xo
    W = torch.zeros((n, K), device="cuda", requires_grad=True)
    mm, vv = torch.zeros_like(W), torch.zeros_like(W)
    for step in range(1, steps + 1):
        x = torch.einsum("npk,nk->np", Dm, W) + dc
        loss = torch.nn.functional.softplus(-x.clamp(-80.0, 1e8)).sum() + REG * npairs * (W * W).sum()
        g, = torch.autograd.grad(loss, W)
        lr_t = LR * np.sqrt(1 - B2 ** step) / (1 - B1 ** step)
        with torch.no_grad():
            mm.mul_(B1).add_(g, alpha=1 - B1)
            vv.mul_(B2).addcmul_(g, g, value=1 - B2)
            W -= lr_t * mm / (vv.sqrt() + EPS)
    return W.detach()


def cost(a, results):
    U, I, n = 20_000, 2048, a.items
    rs = np.random.RandomState(0)
    t = af_tables(rs, U, I)
    e = af_engine(t, random_inputs(rs, I), U, I)
    plain = Engine(model="bprmf", num_users=U, num_items=I, embed_k=K, optimizer="adam_tf23", lr=LR, reg=REG, max_batch=1024)
    plain.bind(t["Gu"], t["Gi"], t["Bi"])
    Cn = e.af_encode_new(*random_inputs(rs, n))
    Call = e.af_encode(np.arange(I))
    td = {nm: e.t[nm] for nm in ("Gu", "Gi") + ATT}
    g = torch.Generator(device="cuda").manual_seed(0)
    for npairs in a.pairs:
        ptr = np.arange(n + 1, dtype=np.int64) * npairs               # (on the host: the engine reads its last entry)
        user = torch.randint(U, (n * npairs,), generator=g, device="cuda", dtype=torch.int32)
        other = torch.randint(I, (n * npairs,), generator=g, device="cuda", dtype=torch.int32)
        role = (torch.arange(n * npairs, device="cuda", dtype=torch.int32) & 1).contiguous()
        base = {"items": n, "pairs_per_item": npairs, "steps": a.steps, "optimizer": "adam_tf23", "users": U, "catalogue": I,
                "embed_k": K, "width": H}
        Gi, Bi = torch.zeros((n, K), device="cuda"), torch.zeros(n, device="cuda")

        def fold(steps):
            Gi.zero_()
            e.af_fold_in_items(ptr, user, other, role, steps, Cn, Gi, lr=LR, reg=REG, optimizer="adam_tf23", want_loss=False)

        r = dict(base, case="af_fold_in_items")
        r.update(windows(lambda: fold(a.steps), a.reps))
        rows = Gi.clone()
        one = windows(lambda: fold(1), a.reps)
        fit = (r["ms"] - one["ms"]) * a.steps / max(1, a.steps - 1)
        r.update(ms_one_step=one["ms"], fit_ms=round(fit, 4), pairs_ms=round(r["ms"] - fit, 4))
        rt = dict(base, case="torch")
        rt.update(windows(lambda: torch_fold(td, Call, Cn, user, other, role, n, npairs, a.steps), max(1, a.reps // 2), passes=3))
        rt["max_abs_difference_to_kernel"] = float((torch_fold(td, Call, Cn, user, other, role, n, npairs, a.steps) - rows).abs().max().item())

        def fold_plain():
            Gi.zero_(); Bi.zero_()
            plain.fold_in_items(ptr, user, other, role, a.steps, Gi, Bi, None, lr=LR, reg=REG, optimizer="adam_tf23", want_loss=False)

        rp = dict(base, case="fold_in_items", note="bprx_fold_in_items on a BPRMF handle, the same k and pairs")
        rp.update(windows(fold_plain, a.reps))
        r["torch_over_kernel"] = round(rt["ms"] / r["ms"], 2)
        r["over_bprmf_fold_in_items"] = round(r["ms"] / rp["ms"], 2)
        for x in (r, rt, rp):
            print(json.dumps(x), flush=True)
            results.append(x)
    # the transposed store: the same number of (user, item) pairs through both blocks
    nu, nq = 4096, 4096 * I // U                                      # 4 096 users x I items == nq items x U users
    nu = nq * U // I
    base = {"case": "blocks", "pairs": nu * I, "users": U, "catalogue": I, "embed_k": K, "width": H}
    for alpha in (True, False):
        x, al = torch.empty((nu, I), device="cuda"), (torch.empty((nu, I, 3), device="cuda") if alpha else None)
        xt, alt = torch.empty((nq, U), device="cuda"), (torch.empty((nq, U, 3), device="cuda") if alpha else None)
        p = lambda v: None if v is None else v.data_ptr()
        lib, st = e.lib, torch.cuda.current_stream().cuda_stream
        rs_ = dict(base, form="af_score_block", alpha=alpha, **windows(lambda: lib.bprx_af_score_block(e.h, 0, nu, p(x), p(al), st), a.reps))
        ra = dict(base, form="af_audience_block", alpha=alpha,
                  **windows(lambda: lib.bprx_af_audience_block(e.h, None, None, I, 0, nq, p(xt), p(alt), st), a.reps))
        ra["over_score_block"] = round(ra["ms"] / rs_["ms"], 3)
        ra["same_bits_transposed"] = bool(torch.equal(e.af_score_block(0, U)[0][:, :nq].T.contiguous().view(torch.int32), xt.view(torch.int32)))
        for r in (rs_, ra):
            print(json.dumps(r), flush=True)
            results.append(r)
    for eng in (e, plain):
        eng.sync_check()
        eng.close()


CLUSTERS, SEED = 20, 7


def cluster_inputs(num_items, noise, seed):
    cluster = np.random.RandomState(SEED).randint(CLUSTERS, size=num_items)     # make_interactions_clustered's first draw
    rs = np.random.RandomState(seed)
    strokes = rs.random_sample((CLUSTERS, 28, 28)) < 0.15
    flip = rs.random_sample((num_items, 28, 28)) < 0.05 * noise
    ed = (np.logical_xor(strokes[cluster], flip).astype(np.uint8) * np.uint8(220)).repeat(8, 1).repeat(8, 2)
    col = np.abs(rs.standard_normal((CLUSTERS, DC))[cluster] + noise * rs.standard_normal((num_items, DC))).astype(np.float32)
    cl = np.zeros((num_items, DK), np.float32)
    known = rs.random_sample(num_items) < 0.7
    cl[np.arange(num_items), np.where(known, cluster % DK, rs.randint(DK, size=num_items))] = 1.0
    return ed, col / np.abs(col).max(1, keepdims=True), cl


def metrics(rows, fold, rest, topk):
    hr, cnt = 0.0, 0
    for j in range(rows.shape[0]):
        if not rest[j]:
            continue
        row = rows[j].astype(np.float64).copy()
        row[fold[j]] = -np.inf
        sc = row[rest[j]]
        row[rest[j]] = -np.inf
        for s in sc:
            hr += int((row > s).sum()) < topk
            cnt += 1
    return round(hr / max(cnt, 1), 4), cnt


def quality(a, results):
    U, I, k, h, B = 1500, 400, 32, 32, 512
    tr, _, _ = synth.make_interactions_clustered(U, I, per_user=22, clusters=CLUSTERS, seed=SEED)
    inputs = cluster_inputs(I, 1.0, seed=11)
    held = np.arange(9, I, 10)
    cat = np.setdiff1d(np.arange(I), held)
    new_id = np.full(I, -1, np.int64)
    new_id[cat] = np.arange(cat.size)
    is_held = np.zeros(I, bool)
    is_held[held] = True
    lists_cat = [[int(new_id[i]) for i in l if not is_held[i]] for l in tr]
    owners = [[] for _ in range(I)]
    for u, l in enumerate(tr):
        for i in l:
            owners[i].append(u)
    rs = np.random.RandomState(3)
    order = [list(rs.permutation(owners[int(j)])) for j in held]

    def train(lists, items):
        t = af_tables(np.random.RandomState(0), U, len(items), k, h)
        e = af_engine(t, tuple(np.ascontiguousarray(x[items]) for x in inputs), U, len(items), optimizer="adam_tf23", lr=1e-3, reg=1e-4,
                      B=B, k=k)
        smp = PhiloxSampler(lists, len(items), seed=1).feeds(e)
        for _ in range(a.train_steps):
            e.step(*smp.sample(B), want_loss=False)
        e.sync_check()
        return e

    e = train(lists_cat, cat)
    n = held.size
    Cn = e.af_encode_new(*(np.ascontiguousarray(x[held]) for x in inputs))
    for m in (2, 5, 20):
        ok = [len(o) > m for o in order]
        fold = [o[:m] if good else [] for o, good in zip(order, ok)]
        rest = [o[m:] if good else [] for o, good in zip(order, ok)]
        ptr, user, other, role = draw_item_fold_pairs(fold, lists_cat, cat.size, 4, seed=0)
        Gi = torch.zeros((n, k), device="cuda")
        e.af_fold_in_items(ptr, user, other, role, a.steps, Cn, Gi, lr=0.05, reg=1e-4, optimizer="adam_tf23", want_loss=False)
        warm = e.af_audience_block(0, n, Cn, Gi, want_alpha=False)[0].cpu().numpy()
        hr, cnt = metrics(warm, fold, rest, 20)
        keep = [set() for _ in range(U)]
        for j, f in zip(held, fold):
            for u in f:
                keep[u].add(int(j))
        lists_full = [[i for i in l if not is_held[i] or i in keep[u]] for u, l in enumerate(tr)]
        ec = train(lists_full, np.arange(I))
        full = ec.af_audience_block(0, I, want_alpha=False)[0].cpu().numpy()[held]
        ec.close()
        r = {"case": "quality", "buyers_known": m, "items_evaluated": int(sum(ok)), "relevant_users": cnt, "warm_hr20": hr,
             "trained_in_catalogue_hr20": metrics(full, fold, rest, 20)[0], "random_ranking_hr20": round(20 / U, 4), "users": U,
             "catalogue": int(cat.size), "held_out_items": int(n), "embed_k": k, "width": h, "train_steps": a.train_steps, "batch": B}
        print(json.dumps(r), flush=True)
        results.append(r)
    e.sync_check()
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--pairs", type=int, nargs="+", default=[8, 40, 320])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--train_steps", type=int, default=1500)
    ap.add_argument("--skip", nargs="*", default=[], choices=["cost", "quality"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "af_item_fold_cost.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    results = []
    if "cost" not in a.skip:
        cost(a, results)
    if "quality" not in a.skip:
        quality(a, results)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
