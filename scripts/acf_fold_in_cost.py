"""Cost of folding new users into ACF (bprx_acf_fold_in): n = 4 096 new users x 20 history items x 4 negatives (80 pairs each),
T = 30 sgd steps, I = 20 000 items, M = 49, C = 512, k = 128, h = a = 64, bf16 features.

  acf_fold_in      ms per call = a timed window of --reps calls / reps, the median of five windows with (min, max), for the default
                   form (a user's first pair differences kept in LDS) and for BPRX_FOLD_CACHE=0 (every pair gathered every step),
                   each in an engine of its own (the variable is read at create).  One more call with the library's per-phase HIP
                   events on splits it: `fold_kernel_ms` (k_acf_fold) and `prepare_ms`, the rest of the call (Z / GP of the distinct
                   history items: mark, the MFMA projection, the item vectors); `z_gemm_ms` is the projection alone.
  acf_profile_rows the yardstick (no parent commit has this feature): one forward over the same users and histories, split the same
                   way.  A fold step is one forward plus the pairs plus a backward that recomputes both levels, so
                   `fold_step_over_forward` = fold_kernel_ms / steps / forward_kernel_ms says whether the kernel is in the expected
                   range (a recomputing backward reads Z about twice as often as the forward).
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/acf_fold_in_cost.py [--out profiles/acf_fold_in_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd import _ffi  # noqa: E402
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402

U, M, C, K, H, A = 64, 49, 512, 128, 64, 64


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


def phases(e, fn):
    """One call with the per-phase events on: (wall ms, {phase: ms})."""
    e.profile(True)
    e.profile_read()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    ph = {p: ms for p, (ms, _) in e.profile_read().items()}
    e.profile(False)
    return a.elapsed_time(b), ph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--positives", type=int, default=20)
    ap.add_argument("--negatives", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=2, help="calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acf_fold_in_cost.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    items, n, P = a.items, a.users, a.positives * a.negatives
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, generator=g, device="cuda") * 2 - 1
    glorot = lambda r, c: rnd(r, c) * float(np.sqrt(6.0 / (r + c)))
    F = torch.empty((items, M, C), dtype=torch.bfloat16, device="cuda")
    for i0 in range(0, items, 2000):                             # relu-like maps, half of them zero
        blk = torch.rand((min(2000, items - i0), M, C), generator=g, device="cuda")
        F[i0:i0 + blk.shape[0]] = (blk * (blk > 0.5)).bfloat16()
    w = {"component.W_0_u": glorot(K, H), "component.W_0_i": glorot(C, H), "component.b_0": rnd(H) * 0.1, "component.W_1": glorot(1, H),
         "component.b_1": rnd(1), "item.W_0_u": glorot(K, A), "item.W_0_iv": glorot(K, A), "item.W_0_ip": glorot(K, A),
         "item.W_0_ix": glorot(C, A), "item.b_0": rnd(A) * 0.1, "item.W_1": glorot(1, A), "item.b_1": rnd(1)}
    assert set(w) == set(_ffi.ACF_WEIGHTS)
    Gu, Gi, Pi = glorot(U, K), rnd(items, K) * 0.3, rnd(items, K) * 0.1
    hist = torch.randint(items, (n, a.positives), generator=g, device="cuda", dtype=torch.int32)
    hcsr = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * a.positives, hist.reshape(-1).contiguous())
    ptr = torch.arange(n + 1, dtype=torch.int64, device="cuda") * P
    pos = hist.repeat_interleave(a.negatives, 1).reshape(-1).contiguous()
    neg = torch.randint(items, (n * P,), generator=g, device="cuda", dtype=torch.int32)
    rows = torch.zeros((n, K), device="cuda")
    results, fitted = [], {}
    for form, env in (("lds", None), ("regather", "0")):
        if env is None:
            os.environ.pop("BPRX_FOLD_CACHE", None)
        else:
            os.environ["BPRX_FOLD_CACHE"] = env
        e = Engine(model="bprmf", num_users=U, num_items=items, embed_k=K, feat_dtype="bf16", optimizer="sgd", lr=0.05, reg=1e-3,
                   max_batch=4096)
        e.bind_acf(Gu, Gi, torch.zeros(items), F, Pi, w, [[] for _ in range(U)])

        def fold():
            rows.zero_()
            e.acf_fold_in(ptr, pos, neg, a.steps, rows, csr=hcsr, lr=0.05, reg=1e-3, optimizer="sgd", want_loss=False)

        r = {"case": "acf_fold_in", "form": form, "users": n, "history": a.positives, "pairs_per_user": P, "steps": a.steps,
             "optimizer": "sgd", "items": items, "M": M, "C": C, "embed_k": K, "h": H, "a": A, "features": "bf16"}
        r.update(windows(fold, a.reps))
        wall, ph = phases(e, fold)
        r["fold_kernel_ms"] = round(ph.get("triplet_grad", 0.0), 4)
        r["prepare_ms"] = round(wall - ph.get("triplet_grad", 0.0), 4)
        r["z_gemm_ms"] = round(ph.get("proj_fwd", 0.0), 4)
        r["users_per_s"] = round(n / (r["ms"] * 1e-3), 1)
        fitted[form] = rows.clone()
        if form == "lds":
            y = {"case": "acf_profile_rows", "users": n, "history": a.positives}
            y.update(windows(lambda: e.acf_profile_rows(rows, csr=hcsr), a.reps))
            wall, ph = phases(e, lambda: e.acf_profile_rows(rows, csr=hcsr))
            y["forward_kernel_ms"] = round(ph.get("triplet_grad", 0.0), 4)
            y["prepare_ms"] = round(wall - ph.get("triplet_grad", 0.0), 4)
            r["fold_step_over_forward"] = round(r["fold_kernel_ms"] / a.steps / max(y["forward_kernel_ms"], 1e-9), 3)
        print(json.dumps(r), flush=True)
        results.append(r)
        if form == "lds":
            print(json.dumps(y), flush=True)
            results.append(y)
        e.sync_check()
        e.close()
    os.environ.pop("BPRX_FOLD_CACHE", None)
    results[0]["ratio_to_regather"] = round(results[0]["ms"] / results[-1]["ms"], 3)
    results[0]["same_bits_as_regather"] = bool(torch.equal(fitted["lds"].view(torch.int32), fitted["regather"].view(torch.int32)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
