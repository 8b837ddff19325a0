"""Cost of fitting warm items (bprx_fold_in_items) on the C2 shape of DESIGN.md: 100 000 users, I = 50 000, k = d = 64.

  n = 1 024 new items with 8, 40 and 320 pairs each (roles alternate), T = 30 steps, adam_tf23: ms per call = a timed window of
  --reps calls / reps, the median of five windows with (min, max), in three forms:
    lds        the default: D_p / dc_p of the pairs that fit the wave's LDS share are formed once
    regather   BPRX_FOLD_CACHE=0: every step forms every pair again (an engine of its own: the variable is read at create)
    torch      a batched torch-GPU autograd baseline of the same loss: D and dc of all items formed once with gathers and a batched
               dot, then T steps of loss.backward() and the same sparse-rule Adam on a [n, k + 1] leaf
  and bprx_fold_in on the same pair counts (1 024 new users), the user-side twin.  same_bits_as_regather: the two kernel forms'
  rows, bit for bit.
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/warm_items_cost.py [--out profiles/warm_items_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402

U, I, K, DD, D = 100_000, 50_000, 64, 64, 64
LR, REG, CNEG, B1, B2, EPS = 0.05, 1e-3, 0.1, 0.9, 0.999, 1e-7


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


def torch_fold(t, P, Pn, user, other, role, n, npairs, steps):
    """The definition of include/bprx.h with autograd, all items in one batch; returns W [n, k + 1]."""
    u, o = user.long().view(n, npairs), other.long().view(n, npairs)
    s = 1.0 - 2.0 * role.float().view(n, npairs)
    gu = t["Gu"][u]                                                   # [n, np, k]
    v = (t["Tu"][u] * (Pn[:, None, :DD] - P[o][:, :, :DD])).sum(-1) + (Pn[:, None, DD] - P[o][:, :, DD]) - t["Bi"][o] - (gu * t["Gi"][o]).sum(-1)
    Dm = torch.cat([gu, torch.ones_like(v)[:, :, None]], -1) * s[:, :, None]
    dc = s * v
    npos = (role.view(n, npairs) == 0).sum(1).float()
    rv = torch.full((n, K + 1), float(npairs), device="cuda")
    rv[:, K] = npos + CNEG * (npairs - npos)
    W = torch.zeros((n, K + 1), device="cuda", requires_grad=True)
    m, vv = torch.zeros_like(W), torch.zeros_like(W)
    for step in range(1, steps + 1):
        x = torch.einsum("npk,nk->np", Dm, W) + dc
        loss = torch.nn.functional.softplus(-x.clamp(-80.0, 1e8)).sum() + REG * (rv * W * W).sum()
        g, = torch.autograd.grad(loss, W)
        lr_t = LR * np.sqrt(1 - B2 ** step) / (1 - B1 ** step)
        with torch.no_grad():
            m.mul_(B1).add_(g, alpha=1 - B1)
            vv.mul_(B2).addcmul_(g, g, value=1 - B2)
            W -= lr_t * m / (vv.sqrt() + EPS)
    return W.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1024, help="new items (and new users of the bprx_fold_in rows)")
    ap.add_argument("--pairs", type=int, nargs="+", default=[8, 40, 320])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warm_items_cost.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, generator=g, device="cuda") * 2 - 1
    lim = lambda r, c: float(np.sqrt(6.0 / (r + c)))
    t = dict(Gu=rnd(U, K) * lim(U, K), Gi=rnd(I, K) * lim(I, K), Bi=rnd(I) * 0.1, Tu=rnd(U, DD) * lim(U, DD),
             E=rnd(D, DD) * lim(D, DD), Bp=rnd(D) * lim(D, 1), F=torch.rand((I, D), generator=g, device="cuda"))
    n = a.items
    Fn = torch.rand((n, D), generator=g, device="cuda")
    engines = {}
    for form, env in (("lds", None), ("regather", "0")):
        if env is None:
            os.environ.pop("BPRX_FOLD_CACHE", None)
        else:
            os.environ["BPRX_FOLD_CACHE"] = env
        engines[form] = Engine(model="vbpr", num_users=U, num_items=I, embed_k=K, embed_d=DD, feat_dim=D, feat_dtype="fp32",
                               optimizer="adam_tf23", lr=LR, reg=REG, max_batch=4096).bind(**t)
    os.environ.pop("BPRX_FOLD_CACHE", None)
    e = engines["lds"]
    P, Pn = e.project_rows(t["F"]), e.project_rows(Fn)
    Pn2 = engines["regather"].project_rows(Fn)
    results = []
    for npairs in a.pairs:
        ptr = torch.arange(n + 1, dtype=torch.int64, device="cuda") * npairs
        user = torch.randint(U, (n * npairs,), generator=g, device="cuda", dtype=torch.int32)
        other = torch.randint(I, (n * npairs,), generator=g, device="cuda", dtype=torch.int32)
        role = (torch.arange(n * npairs, device="cuda", dtype=torch.int32) & 1).contiguous()
        rows = {}
        base = {"items": n, "pairs_per_item": npairs, "steps": a.steps, "optimizer": "adam_tf23", "users": U, "catalogue": I,
                "embed_k": K, "embed_d": DD}
        for form in ("lds", "regather"):
            eng, pn = engines[form], (Pn if form == "lds" else Pn2)
            Gi, Bi = torch.zeros((n, K), device="cuda"), torch.zeros(n, device="cuda")

            def fold():
                Gi.zero_(); Bi.zero_()
                eng.fold_in_items(ptr, user, other, role, a.steps, Gi, Bi, pn, lr=LR, reg=REG, optimizer="adam_tf23", want_loss=False)

            r = dict(base, case="fold_in_items", form=form)
            r.update(windows(fold, a.reps))
            rows[form] = torch.cat([Gi, Bi[:, None]], 1).clone()
            results.append(r)
        same = bool(torch.equal(rows["lds"].view(torch.int32), rows["regather"].view(torch.int32)))
        r = dict(base, case="fold_in_items", form="torch")
        r.update(windows(lambda: torch_fold(t, P, Pn, user, other, role, n, npairs, a.steps), max(1, a.reps // 2), passes=3))
        W = torch_fold(t, P, Pn, user, other, role, n, npairs, a.steps)
        r["max_abs_difference_to_kernel"] = float((W - rows["lds"]).abs().max().item())
        results.append(r)
        Gu, Tu = torch.zeros((n, K), device="cuda"), torch.zeros((n, DD), device="cuda")

        def fold_users():
            Gu.zero_(); Tu.zero_()
            e.fold_in(ptr, other, user % I, a.steps, Gu, Tu, lr=LR, reg=REG, optimizer="adam_tf23", want_loss=False)

        ru = dict(base, case="fold_in", form="lds", note="bprx_fold_in, %d new users with the same pair counts" % n)
        ru.update(windows(fold_users, a.reps))
        results.append(ru)
        lds, reg_, tor = results[-4], results[-3], results[-2]
        lds["same_bits_as_regather"] = same
        lds["ratio_to_regather"] = round(lds["ms"] / reg_["ms"], 3)
        lds["torch_over_kernel"] = round(tor["ms"] / lds["ms"], 2)
        lds["kernel_over_fold_in"] = round(lds["ms"] / ru["ms"], 3)
        for r in results[-4:]:
            print(json.dumps(r), flush=True)
    for eng in engines.values():
        eng.sync_check()
        eng.close()
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
