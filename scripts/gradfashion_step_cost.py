"""Cost of GradFashion's factored dense stage: ms per bprx_step of GradFashion (Dc = 1024, De = 3072, ec = ee = 32) against
VBPR (D = 4096) at the C2 shape (U 100 000, I 50 000, k = d = 64, bf16 features, B = 65 536), same batches, sgd.
Prints one JSON line.  Usage: python scripts/gradfashion_step_cost.py [--steps 200] [--warmup 20]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402


def run(factored, steps, warmup, U=100_000, I=50_000, k=64, d=64, B=65_536, Dc=1024, De=3072, ec=32, ee=32):
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    r = lambda *s: (torch.rand(*s, generator=g, device="cuda") - 0.5) * 0.1
    D = Dc + De
    F = torch.rand(I, D, generator=g, device="cuda").mul_(torch.rand(I, D, generator=g, device="cuda") < 0.5).to(torch.bfloat16)
    e = Engine(model="vbpr", num_users=U, num_items=I, embed_k=k, embed_d=d, feat_dim=D, feat_dtype="bf16", optimizer="sgd",
               lr=1e-3, reg=1e-4, max_batch=B)
    if factored:
        e.bind_factored(r(U, k), r(I, k), torch.zeros(I, device="cuda"), r(U, d), F, r(Dc, ec), r(De, ee), r(ec + ee, d),
                        r(ec + ee), Dc, De)
    else:
        e.bind(Gu=r(U, k), Gi=r(I, k), Bi=torch.zeros(I, device="cuda"), Tu=r(U, d), F=F, E=r(D, d), Bp=r(D))
    batches = [tuple(torch.randint(0, n, (B,), generator=g, device="cuda", dtype=torch.int32) for n in (U, I, I))
               for _ in range(8)]
    for s in range(warmup):
        e.step(*batches[s % 8], want_loss=False)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for s in range(steps):
        e.step(*batches[s % 8], want_loss=False)
    b.record()
    b.synchronize()
    e.sync_check()
    ms = a.elapsed_time(b) / steps
    e.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    vbpr = run(False, a.steps, a.warmup)
    gf = run(True, a.steps, a.warmup)
    print(json.dumps({"shape": "C2 bf16 B=65536", "steps": a.steps, "vbpr_ms_per_step": round(vbpr, 4),
                      "grad_fashion_ms_per_step": round(gf, 4), "extra_us": round((gf - vbpr) * 1000, 1)}))


if __name__ == "__main__":
    main()
