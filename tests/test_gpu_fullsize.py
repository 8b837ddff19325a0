"""BASELINE.json configs[1], [3] (per-GPU shard) and [4] at FULL size -- VBPR k=d=64 bf16 100K x 50K; VBPR k=d=128 bf16
250K x 62.5K (the c4shard shape: the 9-tile forward, the 8-wave backward with three tiles in flight); VBPR k=d=256 fp8
(17 column tiles, the one-pass scaled-fp8 forward) at the cache-resident size (c5small: 100K x 50K, 205-MB table), at HBM
scale (c5: 1M x 500K, a 2-GB table streamed with `nt` loads, B = 262 144) and in list mode at that scale (c5list: B = 65 536,
the projections run over the batch's distinct items) -- and the configs[2] per-GPU shard (BPRMF k=128,
625K x 1M): the oracle cannot run these in seconds, so the HIP path is checked through size-independent properties and
against an independent torch fp32 recomputation of the SAME step on the device with the same operand rounding (torch is
the checker here, never the product path).  Reference: VBPR.py:59-144, BPRMF.py:55-125."""
import numpy as np
import pytest
import torch

import torch_ref as ref
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
NPU = 20                                                      # bench.py --pos-per-user default


def _state(workload):
    import bench
    w = dict(bench.WORKLOADS[workload])
    dev = torch.device("cuda", 0)
    return w, dev, bench.make_state(w, dev, 77, torch)


def _sampler_properties(U, I, B, dev, g):
    """positives are training interactions, negatives are not; the stream is stateless"""
    from fashionvisualexpl_recommend_amd.engine import PhiloxSampler
    npu = 20
    items = torch.randint(I, (U, npu), generator=g, device=dev, dtype=torch.int32).sort(dim=1).values
    indptr = torch.arange(U + 1, device=dev, dtype=torch.int64) * npu
    pos_user = torch.arange(U, device=dev, dtype=torch.int32).repeat_interleave(npu)
    s = PhiloxSampler.from_csr(indptr, items.reshape(-1), pos_user, I, seed=9)
    u, i, j = s.sample(B)
    rows = items[u.long()]
    assert bool((rows == i[:, None]).any(dim=1).all())
    assert not bool((rows == j[:, None]).any(dim=1).any())
    assert int(u.min()) >= 0 and int(u.max()) < U and int(j.min()) >= 0 and int(j.max()) < I
    u2, i2, j2 = s.sample(B, first=0)
    assert torch.equal(u, u2) and torch.equal(i, i2) and torch.equal(j, j2)          # stateless: same slice, same triplets
    return u, i, j


def _bench_csr(U, I, dev, g, zipf_ranked=False):
    """bench.py's synthetic interactions: NPU positives per user, sorted per user; uniform, or Zipf(1.0) popularity with
    item id = popularity rank (--zipf 1 --zipf-ids ranked: the hot items are ids 0, 1, 2, ...; repeats inside a list)."""
    if zipf_ranked:
        wts = 1.0 / torch.arange(1, I + 1, device=dev, dtype=torch.float64)
        cdf = torch.cumsum(wts / wts.sum(), 0)
        r = torch.rand((U, NPU), generator=g, device=dev, dtype=torch.float64)
        items = torch.searchsorted(cdf, r).clamp_(max=I - 1).to(torch.int32).sort(dim=1).values
    else:
        items = torch.randint(I, (U, NPU), generator=g, device=dev, dtype=torch.int32).sort(dim=1).values
    indptr = torch.arange(U + 1, device=dev, dtype=torch.int64) * NPU
    pos_user = torch.arange(U, device=dev, dtype=torch.int32).repeat_interleave(NPU)
    return items, indptr, pos_user


def _epoch_properties(items, I, u, i, j, perm, first):
    """an epoch-walk window [first, first + B) of one epoch: users in the epoch's order, each user's positives once and in
    list order, negatives outside the user's list"""
    B = u.numel()
    pos = torch.arange(first, first + B, device=u.device)
    want_u = perm[pos // NPU]
    assert torch.equal(u.long(), want_u)
    assert torch.equal(i, items[want_u, pos % NPU])
    rows = items[u.long()]
    assert not bool((rows == j[:, None]).any(dim=1).any())
    assert int(j.min()) >= 0 and int(j.max()) < I


@pytest.mark.parametrize("workload", ["c2", "c4shard", "c5small", "c5", "c5list"])
def test_vbpr_full_size_step_against_torch_fp32(workload):
    """i.i.d. batches (PhiloxSampler without .feeds(): the int32 index scan)"""
    _vbpr_full_size_step(workload, "iid")


@pytest.mark.parametrize("workload", ["c2", "c4shard", "c5small", "c5", "c5list"])
def test_vbpr_full_size_step_on_the_epoch_walk(workload):
    """the bench's batches: EpochWalkSampler.from_csr(...).feeds(eng) over its CSR shape, so the step scans the sampler's
    byte planes (index pass kind 2; c5list runs list mode)"""
    _vbpr_full_size_step(workload, "epoch")


def _vbpr_full_size_step(workload, sampler):
    from fashionvisualexpl_recommend_amd.engine import Engine, EpochWalkSampler
    w, dev, t = _state(workload)
    U, I, k, d, D, B = w["U"], w["I"], w["k"], w["d"], w["D"], w["B"]
    fp8 = w["dtype"] == "fp8"
    lr, reg = 1e-3, 1e-4
    g = torch.Generator(device=dev); g.manual_seed(5)
    t["Bi"] = torch.randn(I, generator=g, device=dev) * 0.01
    before = {n: v.clone() for n, v in t.items() if n != "F"}
    eng = Engine(model="vbpr", num_users=U, num_items=I, embed_k=k, embed_d=d, feat_dim=D, feat_dtype=w["dtype"],
                 optimizer="sgd", lr=lr, reg=reg, max_batch=B).bind(**t)
    if sampler == "iid":
        u, i, j = _sampler_properties(U, I, B, dev, g)
    else:                                                     # bench.py's stream: the epoch walk, feeding the byte planes
        items, indptr, pos_user = _bench_csr(U, I, dev, g)
        smp = EpochWalkSampler.from_csr(indptr, items.reshape(-1), pos_user, I, seed=2024).feeds(eng)
        u, i, j = smp.sample(B)
        perm = torch.as_tensor(orc.epoch_perm(2024, 0, U), device=dev).long()
        _epoch_properties(items, I, u, i, j, perm, 0)

    # ---- independent fp32 recomputation of the step (tests/torch_ref.py): the SAME operand rounding (bf16 / e4m3
    # operands of the two projections), fp32 (matmuls) and fp64 (scatter sums) everywhere else ----
    state = dict(before, F=t["F"])
    fwd = ref.vbpr_forward(state, (u, i, j), fp8)
    xp, Eq, frow = fwd["xp"], fwd["Eq"], fwd["frow"]
    ul, il, jl = u.long(), i.long(), j.long()
    got_xp = eng.score_pairs(u, i)
    torch.testing.assert_close(got_xp, xp, rtol=2e-4, atol=2e-4)
    got_blk = eng.score_block(1000, 1064)                      # predict_all rows through the full-table projection
    blk_want = before["Bi"][None, :] + before["Gu"][1000:1064] @ before["Gi"].T
    Pall_d = torch.cat([frow(torch.arange(s0, min(I, s0 + 8192), device=dev)) @ Eq for s0 in range(0, I, 8192)])
    blk_want = blk_want + before["Tu"][1000:1064] @ Pall_d[:, :d].T + Pall_d[:, d][None, :]
    torch.testing.assert_close(got_blk, blk_want, rtol=2e-4, atol=2e-4)
    del Pall_d, blk_want, got_blk
    grads, loss_want = ref.vbpr_grads(state, (u, i, j), reg, fp8, fwd=fwd)
    want = ref.sgd(state, grads, lr)
    dBi = grads["Bi"]
    loss = float(eng.step(u, i, j).item())
    eng.sync_check()
    if sampler == "epoch" and workload != "c5list":
        assert eng.lib.bprx_index_pass_kind(eng.h) == 2, workload       # the bench's step scans the sampler's byte planes
    assert loss == pytest.approx(float(loss_want), rel=2e-4)

    for n in ("Gu", "Tu", "Gi", "Bi", "E", "Bp"):
        wv = want[n]
        delta_scale = float((wv - before[n]).abs().max()) + 1e-12
        err = float((eng.t[n] - wv).abs().max())
        assert err <= 5e-3 * delta_scale + 1e-7, (workload, n, err, delta_scale)      # error relative to the size of the update
    # conservation: with the +g / -g bias gradients, sum(dBi) carries only the regularisation terms
    assert abs(float(dBi.sum()) - float((2 * reg * before["Bi"][il].double()).sum()
                                         + (0.2 * reg * before["Bi"][jl].double()).sum())) < 1e-6 * B
    # a second step from the updated state must keep every table finite and move the loss only slightly
    loss2 = float(eng.step(u, i, j).item())
    eng.sync_check()
    assert np.isfinite(loss2) and abs(loss2 - loss) < 0.05 * abs(loss)


def test_c3_shard_full_size_bprmf_against_torch_fp32():
    from fashionvisualexpl_recommend_amd.engine import Engine
    w, dev, t = _state("c3shard")
    U, I, k, B = w["U"], w["I"], w["k"], w["B"]
    lr, reg = 0.05, 1e-4
    before = {n: v.clone() for n, v in t.items()}
    eng = Engine(model="bprmf", num_users=U, num_items=I, embed_k=k, optimizer="sgd", lr=lr, reg=reg, max_batch=B).bind(**t)
    g = torch.Generator(device=dev); g.manual_seed(6)
    u = torch.randint(U, (B,), generator=g, device=dev, dtype=torch.int32)
    i = torch.randint(I, (B,), generator=g, device=dev, dtype=torch.int32)
    j = torch.randint(I, (B,), generator=g, device=dev, dtype=torch.int32)
    u[:64] = 12345                                           # force some heavily shared rows next to the exclusive majority
    j[100:110] = i[100:110]
    ul = u.long()
    grads, _ = ref.bprmf_grads(before, (u, i, j), reg)
    eng.step(u, i, j)
    eng.sync_check()
    torch.testing.assert_close(eng.t["Gu"], before["Gu"] - lr * grads["Gu"].float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(eng.t["Gi"], before["Gi"] - lr * grads["Gi"].float(), rtol=1e-5, atol=1e-6)
    untouched = torch.ones(U, dtype=torch.bool, device=dev); untouched[ul] = False
    assert torch.equal(eng.t["Gu"][untouched], before["Gu"][untouched])        # rows outside the batch are bit-identical


@pytest.mark.parametrize("layout", ["uniform", "zipf_ranked"])
def test_c2_epoch_walk_steps_in_the_bench_form(layout):
    """bench.py's loop: the epoch-walk sampler built on the default stream, ~32 steps on a side stream with wait_stream,
    want_loss=False on the timed-path step.  c2 has N = 2 000 000 interactions and B = 65 536: batch 30 is filled by two
    sampler calls (epoch 0 -> 1, the epoch prepared one ahead).  Steps 0, 29, 30, 31 are recomputed by the torch restatement
    from a clone of the state just before each of them.  zipf_ranked: Zipf(1.0) popularity with id = rank (bench.py --zipf 1
    --zipf-ids ranked), the hot items' owners overflow their entry regions at full batch size."""
    from fashionvisualexpl_recommend_amd.engine import Engine, EpochWalkSampler
    w, dev, t = _state("c2")
    U, I, k, d, D, B = w["U"], w["I"], w["k"], w["d"], w["D"], w["B"]
    lr, reg, seed = 1e-3, 1e-4, 2024
    g = torch.Generator(device=dev); g.manual_seed(99)
    t["Bi"] = torch.randn(I, generator=g, device=dev) * 0.01
    eng = Engine(model="vbpr", num_users=U, num_items=I, embed_k=k, embed_d=d, feat_dim=D, feat_dtype=w["dtype"],
                 optimizer="sgd", lr=lr, reg=reg, max_batch=B).bind(**t)
    items, indptr, pos_user = _bench_csr(U, I, dev, g, zipf_ranked=layout == "zipf_ranked")
    smp = EpochWalkSampler.from_csr(indptr, items.reshape(-1), pos_user, I, seed=seed).feeds(eng)
    N = U * NPU
    checked = {0: None, 29: None, 30: None, 31: None}
    assert 30 * B < N < 31 * B                               # batch 30 crosses the epoch boundary
    names = ("Gu", "Tu", "Gi", "Bi", "E", "Bp")
    bufs = tuple(torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    run = torch.cuda.Stream(device=dev)
    run.wait_stream(torch.cuda.current_stream())
    kinds = {}
    with torch.cuda.stream(run):
        for s in range(32):
            snap = {n: eng._t[n].clone() for n in names} if s in checked else None
            u, i, j = smp.sample(B, out=bufs)
            loss = eng.step(u, i, j, want_loss=s != 30)
            kinds[s] = eng.lib.bprx_index_pass_kind(eng.h)
            if s in checked:
                checked[s] = (snap, (u.clone(), i.clone(), j.clone()), loss.clone() if s != 30 else None,
                              {n: eng._t[n].clone() for n in names})
    run.synchronize()
    eng.sync_check()
    assert all(kv == 2 for kv in kinds.values()), kinds      # every step, the crossing batch too, scans the byte planes
    perms = [torch.as_tensor(orc.epoch_perm(seed, e, U), device=dev).long() for e in (0, 1)]
    for s, (before, (u, i, j), loss, after) in checked.items():
        # the sampler's side of the step: the epoch-walk window(s) of this batch
        p0 = s * B
        if p0 + B <= N:
            _epoch_properties(items, I, u, i, j, perms[0], p0)
        elif p0 >= N:
            _epoch_properties(items, I, u, i, j, perms[1], p0 - N)
        else:
            cut = N - p0
            _epoch_properties(items, I, u[:cut], i[:cut], j[:cut], perms[0], p0)
            _epoch_properties(items, I, u[cut:], i[cut:], j[cut:], perms[1], 0)
        state = dict(before, F=t["F"])
        grads, loss_want, want = ref.vbpr_step(state, (u, i, j), lr, reg)
        if loss is not None:
            assert float(loss) == pytest.approx(float(loss_want), rel=2e-4), s
        for n in names:
            delta_scale = float((want[n] - before[n]).abs().max()) + 1e-12
            err = float((after[n] - want[n]).abs().max())
            assert err <= 5e-3 * delta_scale + 1e-7, (layout, s, n, err, delta_scale)


@pytest.mark.parametrize("workload", ["c2", "c3shard"])
def test_adam_tf23_full_size_one_and_two_steps(workload):
    """The reference's optimizer at full size: TF-2.3 Adam (non-lazy sparse rows, dense ApplyAdam for E / Bp) from zero
    slots, two epoch-walk batches of the bench's stream, against the torch restatement.  Step 1 from the initial state,
    step 2 from the engine's synced state after step 1: rows the second batch does not touch still move on their momentum."""
    from fashionvisualexpl_recommend_amd.engine import Engine, EpochWalkSampler
    w, dev, t = _state(workload)
    U, I, k, d, D, B = w["U"], w["I"], w["k"], w["d"], w["D"], w["B"]
    vbpr = w["model"] == "vbpr"
    lr, reg = 1e-3, 1e-4
    g = torch.Generator(device=dev); g.manual_seed(8)
    t["Bi"] = torch.randn(I, generator=g, device=dev) * 0.01
    kw = dict(embed_d=d, feat_dim=D, feat_dtype=w["dtype"]) if vbpr else {}
    eng = Engine(model=w["model"], num_users=U, num_items=I, embed_k=k, optimizer="adam_tf23", lr=lr, reg=reg, max_batch=B,
                 **kw).bind(**t)
    items, indptr, pos_user = _bench_csr(U, I, dev, g)
    smp = EpochWalkSampler.from_csr(indptr, items.reshape(-1), pos_user, I, seed=7).feeds(eng)
    restate = (lambda st, b, tt, ab: ref.vbpr_step(st, b, lr, reg, optimizer="adam_tf23", t=tt, absg=ab)) if vbpr else \
        (lambda st, b, tt, ab: ref.bprmf_step(st, b, lr, reg, optimizer="adam_tf23", t=tt, absg=ab))
    # gradient noise scale: fp32 sums in any order for the rows; for E / Bp also the bf16 rounding of W (one ulp, 2^-8)
    noise = {"E": 2.0 ** -7, "Bp": 2.0 ** -7} if vbpr else {}
    for n in ("Gu", "Gi", "Bi", "Tu"):
        noise[n] = 3e-5
    state = {n: v.clone() for n, v in eng.t.items()}
    for step in (1, 2):
        batch = tuple(x.clone() for x in smp.sample(B))
        loss = float(eng.step(*batch).item())
        eng.sync_check()
        got = {n: v.clone() for n, v in eng.t.items() if n != "F"}          # e.t: every pending row caught up first
        absg = {}
        grads, loss_want, want = restate(state, batch, step, absg)
        assert loss == pytest.approx(float(loss_want), rel=2e-4), step
        counts = ref.assert_adam_close(got, want, grads, absg, lr, noise, 1e-3, tag="%s step %d" % (workload, step))
        print(workload, "step", step, "near-cancelling outliers", counts)
        if step == 2:                                          # momentum-only rows: in batch 1, not in batch 2 -- they moved
            only1 = torch.zeros(U, dtype=torch.bool, device=dev)
            only1[prev[0].long()] = True
            only1[batch[0].long()] = False
            assert int(only1.sum()) > 1000
            moved = (got["Gu"][only1] - state["Gu"][only1]).abs().amax(1)
            assert bool((moved > 0).all())
        prev = batch
        state = dict(got, **({"F": t["F"]} if vbpr else {}))
