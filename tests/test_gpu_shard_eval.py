"""Shard-additive evaluation (bprx_eval_pos / _counts / _finish) with W item shards simulated in one process, against the
host evaluator (evaluator._eval_block) on the full score rows and, bit for bit, against single-GPU bprx_eval_users.  Scores take
a few levels only, so ties are everywhere: between negatives and held-out items, among held-out items, across shard
boundaries.  Plus the sharded models with users that hold more than 32 held-out items (two gloo ranks on one GPU)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _csr(lists, dedup=False):
    from fashionvisualexpl_recommend_amd.evaluator import Evaluator
    return Evaluator._device_csr(None, lists, torch.device("cuda"), dedup=dedup)


def _engine(num_users, num_items):
    from fashionvisualexpl_recommend_amd.engine import Engine
    return Engine(model="bprmf", num_users=num_users, num_items=num_items, embed_k=4, optimizer="sgd", max_batch=16, device=0)


def _data(U, I, seed):
    """Quantised scores, train lists with repeated rows, held-out lists of 0, 1, a few, exactly 32 and 33 items, some of them
    also train items."""
    rs = np.random.RandomState(seed)
    scores = (rs.randint(0, 5, size=(U, I)) * 0.5 - 1.0).astype(np.float32)
    train, held = [], []
    for u in range(U):
        tr = rs.choice(I, size=rs.randint(0, I // 3), replace=False).tolist()
        if len(tr) > 2:
            tr += tr[:2]                                    # repeated train rows (the CSR is deduplicated)
        n = [0, 1, 2, 5, 32, 33][u % 6] if u >= 2 else 4
        ev = rs.choice(I, size=n, replace=False).tolist()
        if u % 4 == 1 and ev and tr and tr[0] not in ev:
            ev[0] = tr[0]                                   # a held-out item that is also a train item
        if u == 0:
            scores[u, ev] = scores[u].max()                 # held-out items tied at the top: ties among themselves
        train.append(tr)
        held.append(ev)
    return scores, train, held


@pytest.mark.parametrize("W", [1, 2, 3, 7])
@pytest.mark.parametrize("K", [1, 10, 400])
def test_shard_additive_eval_matches_host_and_single_gpu(W, K):
    from fashionvisualexpl_recommend_amd.evaluator import _eval_block
    from fashionvisualexpl_recommend_amd.sharded import item_range
    U, I = 90, 137                                          # item_range: 137 over 2, 3, 7 ranks leaves the last shard short
    scores, train, held = _data(U, I, seed=W * 100 + K)
    tr_csr, ev_csr = _csr(train, dedup=True), _csr(held)
    S = torch.as_tensor(scores, device="cuda")
    shards = []
    for r in range(W):
        lo, hi = item_range(I, r, W)
        shards.append((lo, _engine(U, hi - lo), S[:, lo:hi].contiguous()))
    if W > 1:
        assert shards[-1][2].shape[1] < shards[0][2].shape[1]
    sp = torch.stack([e.eval_pos(0, U, s, lo, I, ev_csr) for lo, e, s in shards]).sum(0)            # all-reduce(sum)
    cn = torch.stack([e.eval_counts(0, U, s, lo, I, tr_csr, ev_csr, sp) for lo, e, s in shards]).sum(0, dtype=torch.int32)
    got = shards[0][1].eval_finish(0, U, I, ev_csr, sp, cn, K).cpu().numpy()
    single = _engine(U, I)
    want_dev = single.eval_users(0, U, S.clone(), tr_csr, ev_csr, K).cpu().numpy()
    single.sync_check()
    for _, e, _ in shards:
        e.sync_check()
    # the kernel's claim: identical to bprx_eval_users on the concatenated score row, bit for bit
    assert np.array_equal(got, want_dev)
    n = np.array([len(h) for h in held])
    assert (got[n == 0, 0] == -1).all() and (got[n > 32, 0] == -2).all() and (got[(n > 0) & (n <= 32), 0] >= 0).all()
    assert (n == 32).any() and (n == 33).any()
    host = np.array(_eval_block(scores.copy(), 0, train, held, K))                  # users with a held-out list, in order
    dev = got[n > 0]
    keep = n[n > 0] <= 32
    np.testing.assert_allclose(dev[keep], host[keep], rtol=0, atol=1e-12)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _long_lists_dataset(root, name, seed):
    """A clustered dataset in which four users hold 40 test items each (and one of them 35 validation items)."""
    from fashionvisualexpl_recommend_amd import synth
    U, I = 120, 240
    tr, va, te = synth.make_interactions_clustered(U, I, per_user=22, clusters=12, seed=seed)
    rs = np.random.RandomState(seed)
    for u in (3, 50, 61, 119):
        rest = [i for i in range(I) if i not in set(tr[u]) | set(va[u])]
        te[u] = sorted(rs.choice(rest, size=40, replace=False).tolist())
    rest = [i for i in range(I) if i not in set(tr[7]) | set(te[7])]
    va[7] = sorted(rs.choice(rest, size=35, replace=False).tolist())
    synth.write_dataset(root, name, tr, va, te, I, features=synth.make_features(I, 128, seed=seed).astype(np.float64))


def _worker_long(rank, world, port, root, rec):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), BPRX_ONE_GPU="1")
    from fashionvisualexpl_recommend_amd import train_rec
    args = ["--dataset", "long", "--rec", rec, "--world_size", str(world), "--shard", "item" if rec == "vbpr" else "user",
            "--dist_backend", "gloo", "--batch_size", "128", "--epochs", "1", "--embed_k", "16", "--lr", "0.02", "--top_k", "10",
            "--verbose", "-1", "--data_root", root, "--results_root", os.path.join(root, "res")]
    if rec == "vbpr":
        args += ["--embed_d", "8", "--dtype", "fp32"]
    train_rec.train(args)                                  # trains one epoch and evaluates it: no NotImplementedError
    try:
        from fashionvisualexpl_recommend_amd import train_rec as tr
        from fashionvisualexpl_recommend_amd.evaluator import _eval_block
        m = tr._last_model
        assert max(len(l) for l in m.data.test_list) == 40 and max(len(l) for l in m.data.validation_list) == 35
        got = m.metrics(10)
        parts = [None] * world
        dist.all_gather_object(parts, got)
        assert all(p == got for p in parts)                 # every rank returns the same dict
        if rec == "vbpr":
            sc = m.predict_block(0, m.num_users)           # the gathered score rows (rank 0)
        else:
            full = m.full_state()
            if rank == 0:
                from fashionvisualexpl_recommend_amd.engine import Engine
                e = Engine(model="bprmf", num_users=m.num_users, num_items=m.num_items, embed_k=16, optimizer="sgd", max_batch=16,
                           device=0).bind(Gu=full["Gu"], Gi=full["Gi"], Bi=full["Bi"])
                sc = e.score_block(0, m.num_users).cpu().numpy()           # the same score kernel on the gathered tables
        if rank == 0:
            for suf, lst in (("_t", m.data.test_list), ("_v", m.data.validation_list)):
                rows = np.array(_eval_block(sc.copy(), 0, m.data.training_list, lst, 10))
                for q, name in enumerate(("hr", "p", "r", "auc", "ndcg")):
                    assert got[name + suf] == pytest.approx(rows[:, q].mean(), abs=1e-12), name + suf
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("rec", ["vbpr", "bprmf"])
def test_sharded_metrics_with_40_held_out_items(tmp_path, rec):
    """Users with more than 32 held-out items: the device rows come back -2 and the sharded models recompute them on the host
    (ShardedBPRMF from its own full-width rows, ShardedVBPR after an all-gather of those users' columns)."""
    _long_lists_dataset(str(tmp_path), "long", seed=8)
    mp.spawn(_worker_long, args=(2, _free_port(), str(tmp_path), rec), nprocs=2, join=True)
