"""Cost of an ACF step (bprx_step on an ACF-bound BPRMF handle) and of one full evaluation pass: U = 100 000, I = 50 000, 20
training items per user, feature maps M = 49 x C = 512, k = 128, h = a = 64, reg > 0, adam_tf23; fp32 and bf16 features, B = 256
(the reference default) and B = 65 536.  The per-item projection Z_l = f_l [W_0_i | W_0_ix] is timed with the library's per-kernel
events (phase proj_fwd) and reported against its roofline (f32 MFMA 157 TF for fp32 features, 8 TB/s of feature bytes for bf16).
An ACF step reports its kernels under the library's phase names: proj_fwd = k_acf_proj_*, triplet_grad = k_acf_user,
item_seg = k_acf_triplet, dense_update = k_acf_dense, apply = k_adam_sweep / k_acf_apply_sgd, row_count = k_acf_mark.
--gradient full measures the full-gradient mode (bprx_acf_set_gradient); its extra kernels report as reduce_parts = k_acf_q +
k_acf_user_bwd, loss_reduce = k_acf_item_bwd + k_acf_outer + k_acf_colsum + their k_acf_reduce, proj_bwd = k_acf_proj_bwd_* + its
k_acf_reduce + k_acf_clear (per-kernel times: rocprofv3 --kernel-trace --stats, profiles/acf_full_kernel_stats.txt).
ms_per_step is the median of five timed windows of --steps steps, with (min, max).
Prints one JSON line per case.  Usage: python scripts/acf_step_cost.py [--steps 50] [--warmup 5] [--gradient full] [--no-eval]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fashionvisualexpl_recommend_amd import _ffi, synth  # noqa: E402
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402

U, I, M, C, K, H, A = 100_000, 50_000, 49, 512, 128, 64, 64


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


def case(dtype, B, steps, warmup, train, t, F, gradient="detached"):
    e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=K, feat_dtype=dtype, optimizer="adam_tf23", lr=1e-3, reg=1e-4,
               max_batch=B)
    e.bind_acf(t["Gu"], t["Gi"], t["Bi"], F, t["Pi"], {n: t[n] for n in _ffi.ACF_WEIGHTS}, train,
               **({"gradient": "full"} if gradient == "full" else {}))
    rs = np.random.RandomState(1)
    host = [tuple(rs.randint(0, n, B).astype(np.int32) for n in (U, I, I)) for _ in range(4)]
    batches = [tuple(torch.as_tensor(x, device="cuda") for x in b) for b in host]
    distinct = [len(set(i for u in np.unique(b[0]) for i in train[u])) for b in host]
    for s in range(warmup):
        e.step(*batches[s % 4], want_loss=False)
    torch.cuda.synchronize()
    windows = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for s in range(steps):
            e.step(*batches[s % 4], want_loss=False)
        b.record()
        b.synchronize()
        windows.append(a.elapsed_time(b) / steps)
    ms = float(np.median(windows))
    e.profile(True)
    for s in range(steps):
        e.step(*batches[s % 4], want_loss=False)
    prof = e.profile_read()
    e.profile(False)
    e.sync_check()
    nd = float(np.mean([distinct[s % 4] for s in range(steps)]))
    proj_ms = prof["proj_fwd"][0] / max(1, prof["proj_fwd"][1])
    flop = 2.0 * nd * M * C * 128                                   # h + a = 128 columns
    byts = nd * M * C * (4 if dtype == "fp32" else 2)
    roof = 157e12 if dtype == "fp32" else None
    out = {"case": "step", "gradient": gradient, "dtype": dtype, "B": B, "ms_per_step": round(ms, 4),
           "ms_min_max": [round(min(windows), 4), round(max(windows), 4)], "distinct_items": round(nd, 1),
           "proj_ms": round(proj_ms, 4), "proj_tflops": round(flop / proj_ms / 1e9, 1), "proj_tbps": round(byts / proj_ms / 1e9, 2),
           "phases_ms": {k_: round(v[0] / max(1, v[1]), 4) for k_, v in prof.items() if v[1]}}
    out["proj_roofline_frac"] = round((flop / proj_ms * 1e3) / roof, 3) if roof else round((byts / proj_ms * 1e3) / 8e12, 3)
    if gradient == "full" and "proj_bwd" in out["phases_ms"]:       # F^T dZ: the same flops and feature bytes as the forward
        pb = out["phases_ms"]["proj_bwd"]
        out["proj_bwd_tflops"] = round(flop / pb / 1e9, 1)
        out["proj_bwd_tbps"] = round(byts / pb / 1e9, 2)
        out["proj_bwd_roofline_frac"] = round((flop / pb * 1e3) / roof, 3) if roof else round((byts / pb * 1e3) / 8e12, 3)
    print(json.dumps(out), flush=True)
    return e


def evaluation(e, dtype):
    out = torch.empty((4096, I), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for u0 in range(0, U, 4096):
        e.score_block(u0, min(U, u0 + 4096), out[:min(U, u0 + 4096) - u0])
    torch.cuda.synchronize()
    print(json.dumps({"case": "evaluation", "dtype": dtype, "ms": round((time.perf_counter() - t0) * 1e3, 2),
                      "note": "g' of every user (train histories) + predict_all in blocks of 4096 users"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gradient", default="detached", choices=["detached", "full"])
    ap.add_argument("--no-eval", action="store_true", help="skip the evaluation pass")
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--batches", nargs="+", type=int, default=[256, 65_536])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    train, _, _ = synth.make_interactions(U, I, per_user=22, seed=2024)
    rs = np.random.RandomState(0)
    t = tables(rs)
    g = torch.Generator().manual_seed(0)
    F32 = torch.randn((I, M, C), generator=g).abs_()
    for dtype in a.dtypes:
        F = F32 if dtype == "fp32" else F32.to(torch.bfloat16)
        for B in a.batches:
            e = case(dtype, B, a.steps, a.warmup, train, t, F, a.gradient)
            if B == 65_536 and not a.no_eval:
                evaluation(e, dtype)
            e.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
