"""The replicated-user multi-GPU step (ReplicatedUserVBPR.step: overlap form, dense_reduce="gather") with W ranks simulated in
one process: W engines, each bound to its own copy of Gu / Tu / E / Bp and its own item shard, driven one phase at a time, with
the two all-gathers replaced by torch.cat:

  step_begin_sparse -> pack_user_msg -> cat -> step_begin_dense -> apply_user_msgs -> sum_dense_parts(cat of dense parts)
  -> step_end

After a few steps every replica must equal the CPU oracle stepped on the concatenated global batch, the replicas must be
bit-identical (k_msg_link / msg_chain_in_rank_order apply a user's rows in rank order everywhere), and the staging tables
must be left all-zero.  A user sits in every non-empty batch of every step (a chain of W links); some ranks have empty
batches (count-0 messages); under adam_tf23 a user misses a step and comes back (lazy replay)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _batches(W, U, ish, B, step, rs, opt):
    out = []
    for r in range(W):
        nb = B - 5 * r
        if W > 1 and step == 1 and r % 2 == 1:
            nb = 0                                          # an empty batch: count-0 message, zero dense gradient
        u = rs.randint(U, size=nb).astype(np.int32)
        if nb:
            u[0] = 0                                        # user 0: in every rank's batch, every step
            if opt == "adam_tf23" and step != 1:
                u[1] = 5                                    # user 5: absent in step 1, back in step 2 (lazy replay)
        if opt == "adam_tf23" and step == 1:
            u[u == 5] = 6
        out.append((u, rs.randint(ish, size=nb).astype(np.int32), rs.randint(ish, size=nb).astype(np.int32)))
    return out


@pytest.mark.parametrize("W", [1, 3, 4, 8])
@pytest.mark.parametrize("k,d", [(8, 4), (5, 3)])
@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
def test_replicated_user_step_w_ranks_match_oracle(W, k, d, opt):
    from fashionvisualexpl_recommend_amd import synth
    from fashionvisualexpl_recommend_amd.engine import Engine
    from oracle import oracle as orc
    U, I, D, B = 40, 96, 64, 48
    lr, reg = (0.05, 1e-3) if opt == "sgd" else (0.01, 1e-3)
    ish = I // W
    rs = np.random.RandomState(10 * W + k)
    F = synth.make_features(I, D, seed=W)
    F = (F / np.abs(F).max()).astype(np.float32)
    t = dict(Gu=synth.glorot_uniform(rs, U, k), Gi=synth.glorot_uniform(rs, I, k), Bi=(rs.standard_normal(I) * 0.01).astype(np.float32),
             Tu=synth.glorot_uniform(rs, U, d), F=F, E=synth.glorot_uniform(rs, D, d), Bp=synth.glorot_uniform(rs, D, 1).reshape(-1))
    cap = U
    engs, msg = [], []
    for r in range(W):
        it = slice(r * ish, (r + 1) * ish)
        e = Engine(model="vbpr", num_users=U, num_items=ish, embed_k=k, embed_d=d, feat_dim=D, feat_dtype="fp32", optimizer=opt,
                   lr=lr, reg=reg, max_batch=B, device=0, export_user_grad=True, dense_allreduce=True)
        e.bind(Gu=t["Gu"].copy(), Gi=t["Gi"][it].copy(), Bi=t["Bi"][it].copy(), Tu=t["Tu"].copy(), F=t["F"][it].copy(),
               E=t["E"].copy(), Bp=t["Bp"].copy())
        engs.append(e)
        msg.append(torch.zeros(e.user_msg_floats(cap), dtype=torch.float32, device="cuda"))
    o = orc.OracleModel(**{n: v.copy() for n, v in t.items()}, quant=0)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    for step in range(3):
        bs = _batches(W, U, ish, B, step, rs, opt)
        idx = [tuple(dev(x) for x in b) for b in bs]
        for e, (u, i, j) in zip(engs, idx):
            e.step_begin_sparse(u, i, j)
        for e, m, (u, _, _) in zip(engs, msg, idx):
            e.pack_user_msg(u, cap, m)
        msgs = torch.cat(msg)                               # all-gather of the messages
        for e in engs:
            e.step_begin_dense()
        dparts = torch.cat([e.dense_grad() for e in engs])  # all-gather of the dense gradients
        for e in engs:
            e.apply_user_msgs(msgs, W, cap, -lr)
            e.sum_dense_parts(dparts, W)
            e.step_end(want_loss=False)
        o.step(np.concatenate([b[0] for b in bs]), np.concatenate([b[1] + r * ish for r, b in enumerate(bs)]),
               np.concatenate([b[2] + r * ish for r, b in enumerate(bs)]), opt, lr, reg)
    for e in engs:
        e.sync_check()
    rt, at = 2e-5, (2e-6 if opt == "sgd" else max(2e-6, 2e-3 * lr))     # the tolerances of test_gpu_dist.py
    for r, e in enumerate(engs):
        it = slice(r * ish, (r + 1) * ish)
        for n, want in (("Gu", o.Gu), ("Tu", o.Tu), ("E", o.E), ("Bp", o.Bp), ("Gi", o.Gi[it]), ("Bi", o.Bi[it])):
            np.testing.assert_allclose(e.t[n].cpu().numpy(), want, rtol=rt, atol=at, err_msg="%s, rank %d" % (n, r))
    for n in ("Gu", "Tu", "E", "Bp"):                        # the replicas agree bit for bit
        ref = engs[0].t[n].cpu()
        assert all(torch.equal(ref, e.t[n].cpu()) for e in engs[1:]), n
    for r, e in enumerate(engs):
        g, tt = e.user_grad()
        assert float(g.abs().max()) == 0.0 and float(tt.abs().max()) == 0.0, "staging not zero, rank %d" % r
