"""Cost of ACF's explanation read-out (bprx_acf_explain) next to the profile walk it extends (bprx_acf_profiles), on the shape
DESIGN.md section 9 uses for ACF: U = 100 000, I = 50 000, 20 training items per user, feature maps M = 49 x C = 512, k = 128,
h = a = 64; fp32 and bf16 features.  Every user is explained for 20 items (2 000 000 pairs) in blocks of --block users, one
bprx_acf_explain call per block, at top = 1, 5, 32; bprx_acf_profiles runs over the same blocks in the same process.  Both
project Z for the block's distinct history items first (acf_prepare), so the difference is the attention pass's extra store per
entry plus the pair pass.  ms = the median of five timed windows (one pass over all users each), with (min, max).
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/acf_explain_cost.py [--block 4096] [--out profiles/acf_explain_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fashionvisualexpl_recommend_amd import _ffi, synth  # noqa: E402
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402

U, I, M, C, K, H, A, PER_USER = 100_000, 50_000, 49, 512, 128, 64, 64, 20


def tables(rs):
    t = {"Gu": synth.glorot_uniform(rs, U, K), "Gi": synth.glorot_uniform(rs, I, K), "Bi": np.zeros(I, np.float32),
         "Pi": rs.normal(0, 0.01, (I, K)).astype(np.float32)}
    g1 = lambda n: rs.uniform(-np.sqrt(3.0 / n), np.sqrt(3.0 / n), size=n).astype(np.float32)
    shapes = {"component.W_0_u": (K, H), "component.W_0_i": (C, H), "component.b_0": H, "component.W_1": (1, H), "component.b_1": 1,
              "item.W_0_u": (K, A), "item.W_0_iv": (K, A), "item.W_0_ip": (K, A), "item.W_0_ix": (C, A), "item.b_0": A,
              "item.W_1": (1, A), "item.b_1": 1}
    for n in _ffi.ACF_WEIGHTS:
        s = shapes[n]
        t[n] = synth.glorot_uniform(rs, *s) if isinstance(s, tuple) else g1(s)
    return t


def windows(fn, passes=5):
    fn()                                                            # warm-up: workspaces, clocks
    torch.cuda.synchronize()
    out = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"ms": round(float(np.median(out)), 2), "ms_min_max": [round(min(out), 2), round(max(out), 2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=4096, help="users per call")
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--tops", nargs="+", type=int, default=[1, 5, 32])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "acf_explain_cost.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    train, _, _ = synth.make_interactions(U, I, per_user=22, seed=2024)
    rs = np.random.RandomState(0)
    t = tables(rs)
    g = torch.Generator().manual_seed(0)
    F32 = torch.randn((I, M, C), generator=g).abs_()
    items = torch.as_tensor(rs.randint(0, I, (U, PER_USER)).astype(np.int32), device="cuda")
    results = []
    for dtype in a.dtypes:
        F = F32 if dtype == "fp32" else F32.to(torch.bfloat16)
        e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=K, feat_dtype=dtype, optimizer="adam_tf23", lr=1e-3, reg=1e-4,
                   max_batch=256)
        e.bind_acf(t["Gu"], t["Gi"], t["Bi"], F, t["Pi"], {n: t[n] for n in _ffi.ACF_WEIGHTS}, train)
        blocks = []
        for u0 in range(0, U, a.block):
            u = torch.arange(u0, min(U, u0 + a.block), dtype=torch.int32, device="cuda")
            blocks.append((u, u.repeat_interleave(PER_USER), items[u0:u0 + a.block].reshape(-1).contiguous()))

        def profiles():
            for u, _, _ in blocks:
                e.acf_profiles(u)

        r = {"case": "acf_profiles", "dtype": dtype, "users": U, "block": a.block}
        r.update(windows(profiles))
        prof_ms = r["ms"]
        print(json.dumps(r), flush=True)
        results.append(r)
        for top in a.tops:
            def explain():
                for _, uu, ii in blocks:
                    e.acf_explain(uu, ii, top=top)
            r = {"case": "acf_explain", "dtype": dtype, "top": top, "users": U, "pairs": U * PER_USER, "block": a.block}
            r.update(windows(explain))
            r["ratio_to_profiles"] = round(r["ms"] / prof_ms, 3)
            r["us_per_pair"] = round(r["ms"] * 1e3 / (U * PER_USER), 4)
            print(json.dumps(r), flush=True)
            results.append(r)
        e.sync_check()
        e.close()
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
