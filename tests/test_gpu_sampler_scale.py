"""The device samplers at the bench's scale and at their edges, against their CPU twins in oracle/ (bit for bit):
the epoch's keyed Feistel permutation at 1 .. 5 M users and at the power-of-two edges where its domain grows fourfold;
the epoch-walk / Philox streams over the bench's CSR shapes, including the batches that cross an epoch; users that hold
nearly every item (the negative after 1 024 rejections); and the byte-plane index pass at every plane shift edge."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
NPU = 20


@pytest.mark.parametrize("U", [1, 2, 3, 2 ** 20, 2 ** 20 + 1, 100_000, 625_000, 1_000_000, 5_000_000])
def test_epoch_permutation_matches_the_oracle(U):
    from fashionvisualexpl_recommend_amd.engine import EpochWalkSampler
    dev = torch.device("cuda", 0)
    indptr = torch.arange(U + 1, device=dev, dtype=torch.int64)
    items = torch.zeros(U, device=dev, dtype=torch.int32)
    smp = EpochWalkSampler.from_csr(indptr, items, torch.arange(U, device=dev, dtype=torch.int32), 2, seed=2024)
    for epoch in (0, 1, 2):
        perm = smp._prepare(epoch)["perm"]
        assert torch.equal(torch.sort(perm).values, torch.arange(U, device=dev, dtype=torch.int32)), (U, epoch)
        np.testing.assert_array_equal(perm.cpu().numpy(), orc.epoch_perm(2024, epoch, U), err_msg="U %d epoch %d" % (U, epoch))


def _csr(U, I, dev, zipf_ranked=False, seed=99):
    """bench.py's interactions: NPU sorted positives per user, uniform or Zipf(1.0) with id = popularity rank (repeats)"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    if zipf_ranked:
        wts = 1.0 / torch.arange(1, I + 1, device=dev, dtype=torch.float64)
        cdf = torch.cumsum(wts / wts.sum(), 0)
        r = torch.rand((U, NPU), generator=g, device=dev, dtype=torch.float64)
        items = torch.searchsorted(cdf, r).clamp_(max=I - 1).to(torch.int32).sort(dim=1).values
    else:
        items = torch.randint(I, (U, NPU), generator=g, device=dev, dtype=torch.int32).sort(dim=1).values
    indptr = torch.arange(U + 1, device=dev, dtype=torch.int64) * NPU
    pos_user = torch.arange(U, device=dev, dtype=torch.int32).repeat_interleave(NPU)
    return indptr, items.reshape(-1), pos_user


SHAPES = {"c2": (100_000, 50_000, 65_536), "c3shard": (625_000, 1_000_000, 65_536), "c5": (1_000_000, 500_000, 262_144),
          "c2_zipf_ranked": (100_000, 50_000, 65_536)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_epoch_walk_stream_at_bench_scale(shape):
    """First batch, the batch that crosses epoch 0 -> 1 (two kernel calls) and the one that crosses 1 -> 2 (the epoch
    prepared one ahead), bit for bit against orc.sample_epoch; epoch 0's (u, i) pairs are exactly the CSR's interactions."""
    from fashionvisualexpl_recommend_amd.engine import EpochWalkSampler
    U, I, B = SHAPES[shape]
    dev = torch.device("cuda", 0)
    indptr, items, pos_user = _csr(U, I, dev, zipf_ranked=shape.endswith("zipf_ranked"))
    N, seed = U * NPU, 2024
    smp = EpochWalkSampler.from_csr(indptr, items, pos_user, I, seed=seed)
    nb = (2 * N) // B + 1                                   # through the batch that crosses into epoch 2
    want_batches = {0, N // B, (2 * N) // B}
    assert N % B and (2 * N) % B                            # both crossings fall inside a batch
    got, keys = {}, []
    for b in range(nb):
        u, i, j = smp.sample(B)
        if b in want_batches:
            got[b] = (u.cpu().numpy(), i.cpu().numpy(), j.cpu().numpy())
        if b * B < N:
            n = min(B, N - b * B)
            keys.append(u[:n].long() * I + i[:n].long())
    ip, it = indptr.cpu().numpy(), items.cpu().numpy()
    for b, (u, i, j) in got.items():
        parts, p = [], b * B
        while p < (b + 1) * B:                              # the window, split at the epoch boundaries
            e, q = divmod(p, N)
            n = min((b + 1) * B - p, N - q)
            parts.append(orc.sample_epoch_csr(ip, it, I, seed, e, q, n))
            p += n
        for x, name, k in zip((u, i, j), "uij", range(3)):
            np.testing.assert_array_equal(x, np.concatenate([w[k] for w in parts]), err_msg="%s batch %d %s" % (shape, b, name))
    epoch0 = torch.sort(torch.cat(keys)).values
    assert torch.equal(epoch0, torch.sort(pos_user.long() * I + items.long()).values)     # every interaction exactly once


@pytest.mark.parametrize("shape", ["c2", "c5", "c2_zipf_ranked"])
def test_philox_stream_at_bench_scale(shape):
    from fashionvisualexpl_recommend_amd.engine import PhiloxSampler
    U, I, B = SHAPES[shape]
    dev = torch.device("cuda", 0)
    indptr, items, pos_user = _csr(U, I, dev, zipf_ranked=shape.endswith("zipf_ranked"))
    smp = PhiloxSampler.from_csr(indptr, items, pos_user, I, seed=2024)
    host = [a.cpu().numpy() for a in (indptr, items, pos_user)]
    for first in (0, U * NPU - B // 2, (1 << 32) - 100):    # ... and across the 32-bit word of the counter
        got = smp.sample(B, first=first)
        want = orc.sample_philox_csr(*host, I, 2024, first, B)
        for x, w, name in zip(got, want, "uij"):
            np.testing.assert_array_equal(x.cpu().numpy(), w, err_msg="%s first %d %s" % (shape, first, name))


def _dense_lists(I, rs):
    """users 0..2 hold all but 1, 2, 3 of the I items (user 2 with repeated ids); the rest hold a few items"""
    lists = []
    for u, missing in enumerate((1, 2, 3)):
        keep = np.sort(rs.choice(I, I - missing, replace=False))
        if u == 2:
            keep = np.sort(np.concatenate([keep, keep[::97]]))
        lists.append(keep.tolist())
    lists += [sorted(rs.choice(I, 12, replace=False).tolist()) for _ in range(60)]
    return lists


@pytest.mark.parametrize("kind", ["epoch", "philox"])
def test_dense_users_never_draw_a_positive(kind):
    """The reference draws until the negative is not a positive (dataset.py:102).  A user holding 1 999 of 2 000 items
    exhausts the 1 024 rejection draws in ~60 % of its triplets; the fallback must still return a non-positive, uniform over
    the user's non-positives, and the device must agree with the oracle bit for bit."""
    from fashionvisualexpl_recommend_amd.engine import EpochWalkSampler, PhiloxSampler
    I, B = 2000, 1024
    rs = np.random.RandomState(5)
    lists = _dense_lists(I, rs)
    smp = (EpochWalkSampler if kind == "epoch" else PhiloxSampler)(lists, I, seed=11)
    N = sum(len(l) for l in lists)
    sets = [set(l) for l in lists]
    us, js = [], []
    for b in range(3 * N // B + 1):                         # three epochs and more
        u, i, j = (x.cpu().numpy() for x in smp.sample(B))
        us.append(u); js.append(j)
        if b < 2:
            want = orc.sample_epoch(lists, I, 11, 0, b * B, B) if kind == "epoch" else orc.sample_philox(lists, I, 11, b * B, B)
            for x, w, name in zip((u, i, j), want, "uij"):
                np.testing.assert_array_equal(x, w, err_msg="%s batch %d %s" % (kind, b, name))
    u, j = np.concatenate(us), np.concatenate(js)
    assert ((0 <= j) & (j < I)).all()
    bad = [k for k in range(len(u)) if j[k] in sets[u[k]]]
    assert not bad, "%d negatives are positives of their user (first: user %d item %d)" % (len(bad), u[bad[0]], j[bad[0]])
    for user, missing in ((0, 1), (1, 2), (2, 3)):          # uniform over the non-positives
        free = sorted(set(range(I)) - sets[user])
        assert len(free) == missing
        cnt = np.array([(j[u == user] == f).sum() for f in free])
        assert cnt.sum() == (u == user).sum() > 1500
        assert (np.abs(cnt - cnt.mean()) <= 0.15 * cnt.mean()).all(), (user, cnt)


def test_a_user_holding_every_item_is_refused():
    from fashionvisualexpl_recommend_amd.engine import EpochWalkSampler, PhiloxSampler
    I = 300
    dev = torch.device("cuda", 0)
    lists = [list(range(I)), [1, 5, 7]]
    for cls in (PhiloxSampler, EpochWalkSampler):
        with pytest.raises(ValueError):
            cls(lists, I)
        full = torch.cat([torch.arange(I, dtype=torch.int32), torch.tensor([3, 3], dtype=torch.int32),   # repeats count once
                          torch.tensor([1, 5, 7], dtype=torch.int32)]).to(dev)
        indptr = torch.tensor([0, I + 2, I + 5], dtype=torch.int64, device=dev)
        full_sorted = torch.cat([torch.sort(full[:I + 2]).values, full[I + 2:]])
        pos_user = torch.tensor([0] * (I + 2) + [1] * 3, dtype=torch.int32, device=dev)
        with pytest.raises(ValueError):
            cls.from_csr(indptr, full_sorted, pos_user, I)
        ok = torch.cat([full_sorted[:I + 2][full_sorted[:I + 2] != 42], full[I + 2:]])          # one item missing: accepted
        indptr_ok = torch.tensor([0, I + 1, I + 4], dtype=torch.int64, device=dev)
        pos_ok = torch.tensor([0] * (I + 1) + [1] * 3, dtype=torch.int32, device=dev)
        s = cls.from_csr(indptr_ok, ok, pos_ok, I)
        u, i, j = s.sample(64)
        assert not bool(((u == 0) & (j != 42)).any())


def _plane_lists(U, I, sh, rs):
    """lists holding item 0, item I-1 and the first / last item of several owner ranges of 2^sh items"""
    R = 1 << sh if sh else 1 << 13
    owners = (I + R - 1) // R
    edges = {0, I - 1}
    for r in {0, 1, owners // 2, owners - 2, owners - 1}:
        edges.update({min(r * R, I - 1), min((r + 1) * R - 1, I - 1)})
    edges = sorted(edges)
    lists = []
    for u in range(U):
        l = set(rs.choice(I, size=6, replace=False).tolist())
        l.update(edges[u % len(edges)::3])
        lists.append(sorted(l))
    return lists


@pytest.mark.parametrize("kind", ["epoch", "philox"])
@pytest.mark.parametrize("I,shift", [(65_536, 8), (65_537, 9), (262_145, 11), (1_048_576, 12), (1_048_577, 13),
                                     (2_097_152, 13), (2_097_153, 0)])
def test_byte_plane_shift_edges_against_the_oracle(monkeypatch, I, shift, kind):
    """The index pass on the samplers' byte planes at every shift edge: owners of R = 2^shift items, up to R = 8 192 (the
    LDS limit of k_index_seg); 2 097 153 items have no planes (int32 scan).  BPRMF vs the CPU oracle over five steps,
    one of which crosses the epoch boundary."""
    monkeypatch.setenv("BPRX_ITEM_MODE", "2")
    from fashionvisualexpl_recommend_amd import synth
    from fashionvisualexpl_recommend_amd.engine import Engine, EpochWalkSampler, PhiloxSampler
    U, k, B = 64, 8, 512
    rs = np.random.RandomState(I % 1000)
    t = dict(Gu=synth.glorot_uniform(rs, U, k), Gi=synth.glorot_uniform(rs, I, k), Bi=(rs.standard_normal(I) * 0.01).astype(np.float32))
    lr, reg = 0.05, 1e-3
    e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=k, optimizer="sgd", lr=lr, reg=reg, max_batch=B).bind(**t)
    o = orc.OracleModel(**t, quant=0)
    lists = _plane_lists(U, I, shift, rs)
    assert B < sum(len(l) for l in lists) < 4 * B                # five steps cross at least one epoch boundary
    smp = (EpochWalkSampler if kind == "epoch" else PhiloxSampler)(lists, I, seed=8).feeds(e)
    for step in range(5):
        u, i, j = smp.sample(B)
        loss = e.step(u, i, j).item()
        assert e.lib.bprx_index_pass_kind(e.h) == (2 if shift else 1), step
        want = o.step(u.cpu().numpy(), i.cpu().numpy(), j.cpu().numpy(), "sgd", lr, reg)
        assert loss == pytest.approx(want, rel=2e-5), step
        for n in ("Gu", "Gi", "Bi"):
            np.testing.assert_allclose(e.t[n].cpu().numpy().reshape(-1), getattr(o, n).reshape(-1), rtol=2e-5, atol=2e-6,
                                       err_msg="%s %d" % (n, step))
    e.sync_check()
