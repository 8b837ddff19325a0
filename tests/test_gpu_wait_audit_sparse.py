"""The segment-mode sparse kernels after their loads were re-ordered: k_triplet_seg asks for the user's slot and
count beside the other index-dependent loads, in front of the rows; k_item_seg reads its job in one load and keeps the
entries one pair ahead of the rows, clamped to the chunk.  (The uold save at k_triplet_seg's tail was re-ordered too, measured
and taken out again; its paths -- one run inside a workgroup, a cut run, two runs -- stay covered here.)

Segment-mode steps (BPRX_ITEM_MODE=1 with 2B >= I, BPRX_LIST_MODE=0) against the CPU oracle, with the helpers' bounds of
tests/test_gpu_index_queues.py (BPRMF: loss rel 2e-5, tables rtol 2e-5 / atol 2e-6; VBPR on bf16 features: loss rel 1e-4,
tables rtol 2e-3 / atol 1e-4) and, for the adam_tf23 step, those of tests/test_gpu_adam_lazy.py (rtol 2e-4 / atol 2e-5, fp32
features).

Crafted batches, U = 64, I = 48, B = 250 (asserted from the batch itself in _crafted):
  * items with 0, 1, 2, 3, 4, 5 and 7 occurrences -- the boundaries of k_item_seg's pair walk and its odd tail -- one item with
    SEG_CAP + 1 = 65 and one with 130 (hot items of two and three chunks, the last partial);
  * users with a single run inside one workgroup of the triplet kernel (the in-place update), users whose run is cut by a
    workgroup boundary and users with two separate runs, for the shape's T = 256 / G triplets per workgroup;
  * B % 16 != 0 (and B % T != 0 for every T here: 4, 8, 16, 32).
Shapes (k, d): (64, 64) G = 16, two slices of the user row; (8, 4) G = 8, one partial slice; (96, 96) G = 32, three slices, the
last partial; (256, 0) BPRMF, the d = 0 branch, G = 64; one lazy adam_tf23 step at (64, 64): the triplet kernel's mode 1 and
k_item_seg<G, 2>.

Bit equality.  The library keeps no second form of these kernels that sums in the same order (BPRX_ITEM_MODE=0 is the atomic
staging path), so the reference for torch.equal is a recording: tests/golden/wait_audit_sparse.json holds the SHA-256 of every
table after two steps of the library as it was BEFORE the loads were re-ordered, on the deterministic batches of
tests/test_gpu_dense_defer.py (its _batch construction, here for U = 64, I = 48, n = 40: every item used once or as positive
and negative of two identical triplets, users ascending, one run each of 8 at a multiple of 8 or of 5 -- no sum of the step
depends on an order the hardware picks).  Same loads, same arithmetic, same summation order: the hashes must not move."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from fashionvisualexpl_recommend_amd import synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

U, I, B, D = 64, 48, 250, 128
LR, REG = 0.05, 1e-3
SEG_CAP = 64
SHAPES = [(64, 64), (8, 4), (96, 96), (256, 0)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wait_audit_sparse.json")


def _dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32), device="cuda")


def _group(k, d):
    """pick_group (bprx_sparse.hip): lanes per triplet, 16 B per lane."""
    G = 8
    while G < 64 and 4 * G < max(k, d):
        G *= 2
    return G


def _tables(k, d, seed, bf16=True):
    rs = np.random.RandomState(seed)
    t = dict(Gu=synth.glorot_uniform(rs, U, k), Gi=synth.glorot_uniform(rs, I, k),
             Bi=(rs.standard_normal(I) * 0.01).astype(np.float32))
    if d:
        F = synth.make_features(I, D, seed=seed)
        F = (F / np.abs(F).max()).astype(np.float32)
        t.update(Tu=synth.glorot_uniform(rs, U, d), F=orc.bf16_round(F) if bf16 else F, E=synth.glorot_uniform(rs, D, d),
                 Bp=synth.glorot_uniform(rs, D, 1).reshape(-1))
    return t


def _engine(monkeypatch, k, d, t, optimizer="sgd", lr=LR, dtype="bf16", max_batch=B):
    from fashionvisualexpl_recommend_amd.engine import Engine
    monkeypatch.setenv("BPRX_ITEM_MODE", "1")
    monkeypatch.setenv("BPRX_LIST_MODE", "0")
    kw = dict(embed_d=d, feat_dim=D, feat_dtype=dtype) if d else {}
    return Engine(model="vbpr" if d else "bprmf", num_users=U, num_items=I, embed_k=k, optimizer=optimizer, lr=lr, reg=REG,
                  max_batch=max_batch, **kw).bind(**t)


def _runs(u):
    """(user, start, end) of the maximal runs of equal users, in batch order."""
    cut = np.flatnonzero(np.diff(u)) + 1
    starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [len(u)]])
    return [(int(u[s]), int(s), int(e)) for s, e in zip(starts, ends)]


def _crafted(T, seed):
    """One batch with the occurrence counts and user runs of the module docstring, for T triplets per workgroup."""
    rs = np.random.RandomState(seed)
    perm = rs.permutation(I)
    counts = np.zeros(I, np.int64)
    for it, c in zip(perm[:9], (0, 1, 2, 3, 4, 5, 7, SEG_CAP + 1, 2 * SEG_CAP + 2)):
        counts[it] = c
    rest = perm[9:]
    left = 2 * B - int(counts.sum())
    assert len(rest) <= left <= SEG_CAP * len(rest)          # the filler items: ordinary ones (one chunk each)
    counts[rest] = left // len(rest)
    counts[rest[:left % len(rest)]] += 1
    occ = rs.permutation(np.repeat(np.arange(I), counts))
    i, j = occ[:B].astype(np.int32), occ[B:].astype(np.int32)
    # users: runs of these lengths; every fifth run goes to an earlier user (never the one just before it)
    kinds, users, seen, n = [3, 1, 20, 2, 7, 40, 5], [], [], 0
    fresh = list(rs.permutation(U))
    while len(users) < B:
        if n % 5 == 4:
            usr = next(x for x in seen if x != users[-1])
        else:
            usr = int(fresh.pop())
        seen.append(usr)
        users += [usr] * kinds[n % len(kinds)]
        n += 1
    u = np.asarray(users[:B], np.int32)
    # ---- what the batch must hold, asserted from the batch itself
    got = np.bincount(np.concatenate([i, j]), minlength=I)
    for c in (0, 1, 2, 3, 4, 5, 7, SEG_CAP + 1, 2 * SEG_CAP + 2):
        assert (got == c).sum() >= 1, c
    assert got.sum() == 2 * B and B % 16 and B % T
    runs = _runs(u)
    per_user = {}
    for usr, s, e in runs:
        per_user.setdefault(usr, []).append((s, e))
    inside = lambda s, e: s // T == (e - 1) // T
    assert any(len(r) == 1 and inside(*r[0]) for r in per_user.values()), "a user of one run inside one workgroup"
    assert any(not inside(s, e) for _, s, e in runs), "a run cut by a workgroup boundary"
    assert any(len(r) >= 2 for r in per_user.values()), "a user with two separate runs"
    return u, i, j


def _check(e, o, batch, opt, lr, vbpr, rt, at, tag):
    u, i, j = batch
    loss = e.step(_dev(u), _dev(i), _dev(j)).item()
    want = o.step(u, i, j, opt, lr, REG)
    assert loss == pytest.approx(want, rel=1e-4 if vbpr else 2e-5), tag
    for n in (("Gu", "Gi", "Bi", "Tu", "E", "Bp") if vbpr else ("Gu", "Gi", "Bi")):
        np.testing.assert_allclose(e.t[n].cpu().numpy().reshape(-1), getattr(o, n).reshape(-1), rtol=rt, atol=at,
                                   err_msg="%s %s" % (n, tag))


@pytest.mark.parametrize("k,d", SHAPES, ids=["k%d-d%d" % s for s in SHAPES])
def test_crafted_batches_against_the_oracle(monkeypatch, k, d):
    t = _tables(k, d, seed=k + d)
    e = _engine(monkeypatch, k, d, t)
    o = orc.OracleModel(**t, quant=1 if d else 0)
    rt, at = (2e-3, 1e-4) if d else (2e-5, 2e-6)
    for step in range(2):                                   # (the second step: every counter was back at zero)
        _check(e, o, _crafted(256 // _group(k, d), seed=7 + step), "sgd", LR, bool(d), rt, at, "step %d" % step)
    e.sync_check()
    e.close()


def test_crafted_batch_one_lazy_adam_step(monkeypatch):
    """adam_tf23 in its lazy form: k_triplet_seg's mode 1 (the slot and count loads are issued and unused) and k_item_seg<G, 2>."""
    k, d = 64, 64
    monkeypatch.setenv("BPRX_ADAM_LAZY", "1")
    t = _tables(k, d, seed=11, bf16=False)
    e = _engine(monkeypatch, k, d, t, optimizer="adam_tf23", lr=0.01, dtype="fp32")
    o = orc.OracleModel(**t)
    _check(e, o, _crafted(256 // _group(k, d), seed=9), "adam_tf23", 0.01, True, 2e-4, 2e-5, "adam")
    e.sync_check()
    e.close()


def _plain_batch(seed, n=40):
    """tests/test_gpu_dense_defer.py's _batch for U = 64, I = 48: the same step bit for bit on every run."""
    rs = np.random.RandomState(seed)
    perm = rs.permutation(I)
    x = max(0, -(-(2 * n - I) // 3))                       # items that are positive and negative of two identical triplets
    y = 2 * (n - 2 * x)                                     # items used once, in y / 2 ordinary triplets
    assert x + y <= I and 2 * x + y // 2 == n
    pairs = [(it, it) for it in perm[:x]]
    singles = [(perm[x + 2 * q], perm[x + 2 * q + 1]) for q in range(y // 2)]
    lens = [8] * 3 + [5] * 2 + [2] * 3                      # runs of 8 at multiples of 8, then 5 and 2: at most two workgroups each
    assert sum(lens) == n
    users = np.sort(rs.choice(U, size=len(lens), replace=False))
    u, i, j = [], [], []
    for usr, L in zip(users, lens):                         # identical triplets stay inside one run
        p = min(L // 2, len(pairs))
        for a, b in [pairs.pop() for _ in range(p)]:
            u += [usr] * 2; i += [a] * 2; j += [b] * 2
        for _ in range(L - 2 * p):
            a, b = singles.pop()
            u.append(usr); i.append(a); j.append(b)
    assert len(u) == n and not pairs and not singles
    return tuple(np.asarray(v, dtype=np.int32) for v in (u, i, j))


def plain_hashes(monkeypatch, k, d):
    """SHA-256 of every table after two steps on the deterministic batches (also what wrote the golden file)."""
    t = _tables(k, d, seed=100 + k + d)
    e = _engine(monkeypatch, k, d, t, max_batch=64)
    for s in range(2):
        e.step(*(_dev(a) for a in _plain_batch(300 + s)), want_loss=False)
    out = {n: hashlib.sha256(np.ascontiguousarray(e.t[n].cpu().numpy()).tobytes()).hexdigest()
           for n in (("Gu", "Gi", "Bi", "Tu", "E", "Bp") if d else ("Gu", "Gi", "Bi"))}
    e.sync_check()
    e.close()
    return out


@pytest.mark.parametrize("k,d", SHAPES, ids=["k%d-d%d" % s for s in SHAPES])
def test_plain_batches_keep_the_recorded_bits(monkeypatch, k, d):
    with open(GOLDEN) as f:
        want = json.load(f)["k%d-d%d" % (k, d)]
    got = plain_hashes(monkeypatch, k, d)
    assert got == want, [n for n in want if got.get(n) != want[n]]
