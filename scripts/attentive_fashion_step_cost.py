"""Cost of an AttentiveFashion step (bprx_step on a handle bound with bprx_bind_attentive) and of one full evaluation: U = 100 000,
I = 50 000, k = 128, h = 64, Dc = 512, Dk = 64, reg > 0, dropout 0.5, adam_tf23; B = 256 (the reference default) and B = 4 096.
The two conv kernels are timed with the library's per-kernel events (phase proj_fwd = k_af_conv<fwd>, proj_bwd = k_af_conv<bwd>) and
reported against their rooflines: MFMA FLOPs = positions x 32 x 64 x 2 x 3 weight terms per distinct image (backward: the same for
the recomputation plus eight 16x16x32 counting MFMAs per 32 positions) against the 2.5 PF bf16 peak, uint8 bytes against 8 TB/s.
A timed window holds `--seconds` of steps (the step count is sized from a short trial, so B = 256 and B = 4 096 are timed equally
long) and is repeated `--repeats` times: ms_per_step is the median, ms_spread the (min, max) over the repeats.  The pairwise attention kernel k_af_block is timed by events around bprx_af_score_block (item encodings already made)
against the 157 TF f32 MFMA peak: 3 x k x h x 2 FLOP per (user, item).  Prints one JSON line per case.
Usage: python scripts/attentive_fashion_step_cost.py [--seconds 1.0] [--repeats 5] [--warmup 3] [--eval_users 100000]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fashionvisualexpl_recommend_amd import _ffi, synth  # noqa: E402
from fashionvisualexpl_recommend_amd.engine import Engine  # noqa: E402

U, I, K, H, DC, DK = 100_000, 50_000, 128, 64, 512, 64
POS = 224 * 224


def tables(rs):
    g1 = lambda n: rs.uniform(-np.sqrt(3.0 / n), np.sqrt(3.0 / n), size=n).astype(np.float32)
    lim = np.sqrt(6.0 / 1625)
    return {"Gu": synth.glorot_uniform(rs, U, K), "Gi": synth.glorot_uniform(rs, I, K), "Bi": np.zeros(I, np.float32),
            "color.W1": synth.glorot_uniform(rs, DC, 256), "color.b1": np.zeros(256, np.float32), "color.W2": synth.glorot_uniform(rs, 256, K),
            "edges.conv": rs.uniform(-lim, lim, (25, 64)).astype(np.float32), "edges.conv_b": np.zeros(64, np.float32),
            "edges.W2": synth.glorot_uniform(rs, 64, K), "class.W1": synth.glorot_uniform(rs, DK, 256),
            "class.b1": np.zeros(256, np.float32), "class.W2": synth.glorot_uniform(rs, 256, K),
            "attention.W_1": synth.glorot_uniform(rs, K, H), "attention.b_1": g1(H), "attention.W_2": synth.glorot_uniform(rs, H, 1),
            "attention.b_2": g1(1)}


def case(B, seconds, repeats, warmup, t, inputs):
    e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=K, optimizer="adam_tf23", lr=1e-3, reg=1e-4, max_batch=B)
    e.bind_attentive(t["Gu"], t["Gi"], t["Bi"], *inputs, {n: t[n] for n in _ffi.AF_WEIGHTS}, dropout=0.5, seed=1)
    rs = np.random.RandomState(1)
    host = [tuple(rs.randint(0, n, B).astype(np.int32) for n in (U, I, I)) for _ in range(4)]
    batches = [tuple(torch.as_tensor(x, device="cuda") for x in b) for b in host]
    distinct = [len(set(b[1].tolist()) | set(b[2].tolist())) for b in host]
    def window(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for s in range(n):
            e.step(*batches[s % 4], want_loss=False)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n
    for s in range(warmup):
        e.step(*batches[s % 4], want_loss=False)
    torch.cuda.synchronize()
    steps = max(4, 4 * int(round(seconds * 1e3 / window(4) / 4)))   # a multiple of the four batches
    reps = sorted(window(steps) for _ in range(repeats))
    ms = reps[len(reps) // 2]
    psteps = min(steps, 40)
    e.profile(True)
    for s in range(psteps):
        e.step(*batches[s % 4], want_loss=False)
    prof = e.profile_read()
    e.profile(False)
    e.sync_check()
    nd = float(np.mean(distinct))
    fwd_ms = prof["proj_fwd"][0] / max(1, prof["proj_fwd"][1])
    bwd_ms = prof["proj_bwd"][0] / max(1, prof["proj_bwd"][1])
    fwd_flop = nd * POS * 32 * 64 * 2 * 3
    bwd_flop = fwd_flop + nd * (POS / 32) * 8 * (16 * 16 * 32 * 2)
    out = {"case": "step", "B": B, "ms_per_step": round(ms, 4), "ms_spread": [round(reps[0], 4), round(reps[-1], 4)],
           "steps_per_window": steps, "repeats": repeats, "distinct_items": round(nd, 1),
           "conv_fwd_ms": round(fwd_ms, 4), "conv_fwd_mfma_frac_of_2.5PF": round(fwd_flop / (fwd_ms * 1e-3) / 2.5e15, 4),
           "conv_fwd_hbm_frac_of_8TBs": round(nd * POS / (fwd_ms * 1e-3) / 8e12, 5),
           "conv_bwd_ms": round(bwd_ms, 4), "conv_bwd_mfma_frac_of_2.5PF": round(bwd_flop / (bwd_ms * 1e-3) / 2.5e15, 4),
           "phases_ms": {k_: round(v[0] / max(1, v[1]), 4) for k_, v in prof.items() if v[1]}}
    print(json.dumps(out), flush=True)
    return e


def evaluation(e, users, blk=2048):
    sc = torch.empty((blk, I), dtype=torch.float32, device="cuda")
    e.score_block(0, 8, sc[:8])                                      # item encodings (once per parameter state) + warm-up
    torch.cuda.synchronize()
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record()
    e.tables_dirty()
    e.score_block(0, 8, sc[:8])
    b.record()
    for u0 in range(0, users, blk):
        e.score_block(u0, min(users, u0 + blk), sc[:min(users, u0 + blk) - u0])
    c.record()
    c.synchronize()
    enc_ms, blk_ms = a.elapsed_time(b), b.elapsed_time(c)
    flop = float(users) * I * 3 * K * H * 2
    print(json.dumps({"case": "evaluation", "users": users, "encode_all_items_ms": round(enc_ms, 2), "score_blocks_ms": round(blk_ms, 2),
                      "k_af_block_tflops": round(flop / (blk_ms * 1e-3) / 1e12, 2),
                      "k_af_block_frac_of_157TF_f32_mfma": round(flop / (blk_ms * 1e-3) / 157e12, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=U)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    t = tables(np.random.RandomState(0))
    g = torch.Generator(device="cuda").manual_seed(0)
    edges = torch.zeros((I, 224, 224), dtype=torch.uint8, device="cuda")
    for s0 in range(0, I, 5000):                                     # sparse edge maps: ~10 % of the pixels lit
        n = min(5000, I - s0)
        lit = torch.rand((n, 224, 224), generator=g, device="cuda") < 0.1
        edges[s0:s0 + n] = (torch.randint(64, 256, (n, 224, 224), generator=g, device="cuda") * lit).to(torch.uint8)
    color = torch.rand((I, DC), generator=g, device="cuda")
    color = color / color.abs().max(1, keepdim=True).values
    cls = torch.zeros((I, DK), device="cuda")
    cls[torch.arange(I, device="cuda"), torch.randint(0, DK, (I,), generator=g, device="cuda")] = 1.0
    for B in (256, 4096):
        e = case(B, a.seconds, a.repeats, a.warmup, t, (edges, color, cls))
        if B == 4096:
            evaluation(e, a.eval_users)
        e.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
