"""Cost of one similar-items pass over the whole catalogue (bprx_sim_rnorm, bprx_sim_block, bprx_topk_lists) on the C2 shape of
DESIGN.md: I = 50 000 items, k = d = 64, D = 4 096, bf16 features, K = 20 neighbours per item.

A pass walks the catalogue in blocks of ranking.rows_per_block(4096, I) item rows, as BPRMF.similar_items does: one sim_block and
one topk_lists per block (device work only: the download of the lists is the host's).  Three timings per space, each the median
of five windows of --passes passes with (min, max), from device events around work that ends in a synchronise:

  sim_block     every block's bprx_sim_block, nothing else
  ranking       every block's bprx_topk_lists on a block of cosines that is already there
  pass          both, block by block

Beside them the two bounds of DESIGN.md: the fp32-MFMA time of 2 I^2 w flops (w = the width of z) at 157.3 TFLOP/s, and the HBM
time of the I^2 x 4 bytes sim_block writes plus the I^2 x 4 bytes ranking reads back at 8 TB/s; the binding one is the larger.
Prints one JSON line per case and writes them all to --out.
Usage: python scripts/similar_items_cost.py [--out profiles/similar_items_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402
from fashionvisualexpl_recommend_amd.ranking import rows_per_block  # noqa: E402

U, I, K, DD, D = 1_000, 50_000, 64, 64, 4096                       # (the user side plays no part)
HBM_BYTES_PER_S, MFMA_F32_FLOPS = 8e12, 157.3e12
TARGET = 0.5                                                        # the project's design target: share of the binding bound


def windows(fn, reps, passes=5):
    fn()                                                            # warm-up: code objects, the allocator's blocks, clocks
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
    return {"ms": round(float(np.median(out)), 4), "ms_min_max": [round(min(out), 4), round(max(out), 4)], "passes_per_window": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=I, help="catalogue size (a rehearsal takes fewer)")
    ap.add_argument("--feat_dim", type=int, default=D)
    ap.add_argument("--passes", type=int, default=3, help="whole-catalogue passes per timed window")
    ap.add_argument("--top_k", type=int, default=20)
    ap.add_argument("--spaces", nargs="+", default=["visual", "both", "latent"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similar_items_cost.json"))
    a = ap.parse_args()
    n, Df = a.items, a.feat_dim
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, generator=g, device="cuda") * 2 - 1
    lim = lambda r, c: float(np.sqrt(6.0 / (r + c)))
    F = torch.randn((n, Df), generator=g, device="cuda").abs_()
    F *= torch.rand((n, Df), generator=g, device="cuda") < 0.5       # relu-like: about half zeros
    t = dict(Gu=rnd(U, K) * lim(U, K), Gi=rnd(n, K) * lim(n, K), Bi=torch.zeros(n, device="cuda"), Tu=rnd(U, DD) * lim(U, DD),
             E=rnd(Df, DD) * lim(Df, DD), Bp=rnd(Df) * lim(Df, 1), F=(F / F.max()).to(torch.bfloat16))
    del F
    e = Engine(model="vbpr", num_users=U, num_items=n, embed_k=K, embed_d=DD, feat_dim=Df, feat_dtype="bf16", optimizer="sgd",
               lr=0.05, reg=0.0, max_batch=4096).bind(**t)
    blk = rows_per_block(4096, n)
    blocks = [(b0, min(n, b0 + blk)) for b0 in range(0, n, blk)]
    own = [e.csr([[q] for q in range(b0, b1)]) for b0, b1 in blocks]
    out = torch.empty((blk, n), dtype=torch.float32, device="cuda")
    results = []
    for space in a.spaces:
        w = {"latent": K, "visual": DD, "both": K + DD}[space]
        rn = e.sim_rnorm(space)                                     # (P is made current here, once per parameter state)

        def sim_only():
            for b0, b1 in blocks:
                e.sim_block(space, b0, b1, rn, out=out[:b1 - b0])

        def rank_only():
            for (b0, b1), csr in zip(blocks, own):
                e.topk_lists(out[:b1 - b0], csr, a.top_k)

        def both():
            for (b0, b1), csr in zip(blocks, own):
                e.topk_lists(e.sim_block(space, b0, b1, rn, out=out[:b1 - b0]), csr, a.top_k)

        mfma_ms = 2.0 * n * n * w / MFMA_F32_FLOPS * 1e3
        write_ms = n * n * 4 / HBM_BYTES_PER_S * 1e3
        r = {"case": "sim_rnorm", "space": space, "items": n, "width": w}
        r.update(windows(lambda: e.sim_rnorm(space), 20))
        print(json.dumps(r), flush=True)
        results.append(r)
        for case, fn, bound in (("sim_block", sim_only, max(mfma_ms, write_ms)), ("ranking", rank_only, write_ms),
                                ("pass", both, max(mfma_ms, 2 * write_ms))):
            r = {"case": case, "space": space, "dtype": "bf16", "items": n, "width": w, "top_k": a.top_k, "blocks": len(blocks),
                 "rows_per_block": blk}
            r.update(windows(fn, a.passes))
            r.update(mfma_f32_bound_ms=round(mfma_ms, 4), hbm_bound_ms=round((2 if case == "pass" else 1) * write_ms, 4),
                     binding="mfma" if bound == mfma_ms else "hbm", fraction_of_binding_bound=round(bound / r["ms"], 3))
            r["reaches_design_target"] = bool(r["fraction_of_binding_bound"] >= TARGET)
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
