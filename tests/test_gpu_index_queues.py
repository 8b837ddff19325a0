"""The samplers' owner queues (DESIGN §4 "Owner queues"): bprx_sample_*_h leave every 256 triplets' item occurrences sorted by
owner (id >> 8) and the owner workgroups of k_index_seg read their own records instead of scanning the byte planes.

Every step is compared with the CPU oracle on the same triplets, with the bounds of
test_gpu_segments.test_index_pass_on_the_samplers_byte_planes (loss rel 2e-5, tables rtol 2e-5 / atol 2e-6; BPRMF, k = 32).  The
one VBPR run has bf16 features: its bounds are those of test_gpu_segments.test_segment_step_user_runs_and_hot_items for VBPR (loss
rel 1e-4, tables rtol 2e-3 / atol 1e-4: the bf16 images of W and [E|Bp] carry 2^-9 per element, the index pass has no part in them).
bprx_index_pass_kind is 2 on every sampler-fed step; bprx_index_pass_queue tells whether the owners read the queues.  A batch
filled by two sampler calls (epoch crossing) numbers its regions on behind the first call's: the queues serve it too.

Shapes: 4 owners with a partial last one (I = 1000) and a partial last region (B = 400: 144 triplets); 79 owners, the last of 32
items, 8 regions (I = 20 000, B = 2048); skewed lists (long runs of one owner inside a region, hot chunks in k_item_seg); every
fall-back (the caller's own batch, queues of another batch, B % 16 != 0, wide planes, BPRX_INDEX_QUEUE=0).

Mutations of the library that this file was checked to fail on (each built once and run once on MI355X; 14 cases in all):
  * the negatives' records not written (put_queues)                        -> 12 fail: every case but wide planes / policy off
  * a region's last non-empty owner range one slot short (hi - 1)          -> the same 12
  * the partial last region's dead threads ranked (`live` ignored)         -> 7 fail: every epoch case (the call that ends an
                                                                              epoch ends in a partial region) and few_owners[philox-400]
  * the second sampler call of a batch starting again at region 0          -> 6 fail: every case whose epoch sampler crosses
"""
import numpy as np
import pytest
import torch

from fashionvisualexpl_recommend_amd import synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

LR, REG = 0.05, 1e-3


def _tables(U, I, k, d, D, seed):
    rs = np.random.RandomState(seed)
    t = dict(Gu=synth.glorot_uniform(rs, U, k), Gi=synth.glorot_uniform(rs, I, k),
             Bi=(rs.standard_normal(I) * 0.01).astype(np.float32))
    if d:
        F = synth.make_features(I, D, seed=seed)
        F = orc.bf16_round((F / np.abs(F).max()).astype(np.float32))
        t.update(Tu=synth.glorot_uniform(rs, U, d), F=F, E=synth.glorot_uniform(rs, D, d),
                 Bp=synth.glorot_uniform(rs, D, 1).reshape(-1))
    return t


def _lists(U, I, n, seed, always=()):
    rs = np.random.RandomState(seed)
    return [sorted(set(rs.choice(I, size=n, replace=False).tolist()) | set(always)) for _ in range(U)]


def _engine(U, I, B, k=32, d=0, D=0, seed=9):
    from fashionvisualexpl_recommend_amd.engine import Engine
    t = _tables(U, I, k, d, D, seed)
    kw = dict(embed_d=d, feat_dim=D, feat_dtype="bf16") if d else {}
    e = Engine(model="vbpr" if d else "bprmf", num_users=U, num_items=I, embed_k=k, optimizer="sgd", lr=LR, reg=REG, max_batch=B,
               **kw).bind(**t)
    return e, orc.OracleModel(**t, quant=1 if d else 0), t


def _sampler(kind, lists, I, e, seed=3):
    from fashionvisualexpl_recommend_amd.engine import EpochWalkSampler, PhiloxSampler
    return (EpochWalkSampler if kind == "epoch" else PhiloxSampler)(lists, I, seed=seed).feeds(e)


def _check(e, o, batch, want_kind, want_queue, tag, vbpr=False):
    u, i, j = batch
    loss = e.step(u, i, j).item()
    assert (e.lib.bprx_index_pass_kind(e.h), e.lib.bprx_index_pass_queue(e.h)) == (want_kind, want_queue), tag
    want = o.step(u.cpu().numpy(), i.cpu().numpy(), j.cpu().numpy(), "sgd", LR, REG)
    assert loss == pytest.approx(want, rel=1e-4 if vbpr else 2e-5), tag
    rt, at = (2e-3, 1e-4) if vbpr else (2e-5, 2e-6)
    for n in (("Gu", "Gi", "Bi", "Tu", "E", "Bp") if vbpr else ("Gu", "Gi", "Bi")):
        np.testing.assert_allclose(e.t[n].cpu().numpy().reshape(-1), getattr(o, n).reshape(-1), rtol=rt, atol=at,
                                   err_msg="%s %s" % (n, tag))


@pytest.mark.parametrize("B", [512, 400])
@pytest.mark.parametrize("kind", ["epoch", "philox"])
def test_few_owners_partial_last_owner_and_region(kind, B, monkeypatch):
    """I = 1000: 4 owners, the last of 232 items.  B = 400: the second region holds 144 triplets, its other 112 threads stay for
    the barriers and leave no record.  2 100 positives: the epoch sampler fills one of the six batches in two calls."""
    monkeypatch.setenv("BPRX_ITEM_MODE", "2")
    U, I = 300, 1000
    e, o, _ = _engine(U, I, B)
    smp = _sampler(kind, _lists(U, I, 7, seed=2), I, e)
    for step in range(6):
        _check(e, o, smp.sample(B), 2, 1, "%s B=%d step %d" % (kind, B, step))
    e.sync_check()


@pytest.mark.parametrize("kind,model", [("epoch", "bprmf"), ("philox", "bprmf"), ("epoch", "vbpr")])
def test_many_owners(kind, model, monkeypatch):
    """I = 20 000: 79 owners, the last of 32 items; B = 2048: 8 regions, two threads in three of an owner idle.  5 400 positives:
    the third batch crosses the epoch.  VBPR (d = 8, D = 128, bf16): the owners also zero the Wb rows of the untouched items
    and seg_cnt is the projections' mask."""
    monkeypatch.setenv("BPRX_ITEM_MODE", "2")
    monkeypatch.setenv("BPRX_LIST_MODE", "0")              # (VBPR, 2B < I: the touched-item list would take the step)
    U, I, B = 600, 20000, 2048
    vb = model == "vbpr"
    e, o, _ = _engine(U, I, B, d=8 if vb else 0, D=128 if vb else 0, seed=13)
    smp = _sampler(kind, _lists(U, I, 9, seed=4), I, e)
    for step in range(4):
        _check(e, o, smp.sample(B), 2, 1, "%s %s step %d" % (kind, model, step), vbpr=vb)
    e.sync_check()


@pytest.mark.parametrize("kind", ["epoch", "philox"])
def test_skewed_lists(kind, monkeypatch):
    """Every user's list holds item 7 and item I - 1: two positives in seven belong to owner 0 / the last owner (runs of one
    owner inside a region; ~70 occurrences of each of the two items per batch: more than one chunk in k_item_seg)."""
    monkeypatch.setenv("BPRX_ITEM_MODE", "2")
    U, I, B = 300, 1000, 512
    e, o, _ = _engine(U, I, B, seed=21)
    smp = _sampler(kind, _lists(U, I, 5, seed=6, always=(7, I - 1)), I, e)
    for step in range(5):
        _check(e, o, smp.sample(B), 2, 1, "%s step %d" % (kind, step))
    e.sync_check()


@pytest.mark.parametrize("kind", ["epoch", "philox"])
def test_fall_backs_give_the_same_result(kind, monkeypatch):
    monkeypatch.setenv("BPRX_ITEM_MODE", "2")
    U, I, B = 300, 1000, 512
    e, o, _ = _engine(U, I, B)
    smp = _sampler(kind, _lists(U, I, 7, seed=2), I, e)
    rs = np.random.RandomState(2)
    _check(e, o, smp.sample(B), 2, 1, "on the queues")
    own = tuple(torch.as_tensor(rs.randint(n, size=B).astype(np.int32), device="cuda") for n in (U, I, I))
    _check(e, o, own, 1, 0, "caller's own batch")
    a = smp.sample(B)
    b = smp.sample(B)                                       # the queues (and planes) now belong to b
    _check(e, o, a, 1, 0, "queues of another batch")
    _check(e, o, b, 1, 0, "queues dropped by the step in between")
    _check(e, o, smp.sample(B - 8), 1, 0, "B % 16 != 0")
    _check(e, o, smp.sample(B), 2, 1, "back on the queues")
    e.sync_check()


def test_wide_planes_keep_the_scan(monkeypatch):
    """More than 65 536 items: 16-bit locals do not fit a record; the owners scan the planes (kind 2, no queues)."""
    monkeypatch.setenv("BPRX_ITEM_MODE", "2")
    U, I, B = 400, 70000, 1024
    e, o, _ = _engine(U, I, B, seed=11)
    smp = _sampler("epoch", _lists(U, I, 9, seed=4, always=(0, 65536, I - 1)), I, e, seed=8)
    for step in range(2):
        _check(e, o, smp.sample(B), 2, 0, "wide step %d" % step)
    e.sync_check()


def test_policy_off_keeps_the_scan(monkeypatch):
    monkeypatch.setenv("BPRX_ITEM_MODE", "2")
    monkeypatch.setenv("BPRX_INDEX_QUEUE", "0")
    U, I, B = 300, 1000, 512
    e, o, _ = _engine(U, I, B)
    smp = _sampler("epoch", _lists(U, I, 7, seed=2), I, e)
    for step in range(2):
        _check(e, o, smp.sample(B), 2, 0, "policy 0 step %d" % step)
    e.sync_check()


def test_queue_form_against_plane_form(monkeypatch):
    """Two engines, same tables, same sampler seed, three steps: one on the queues, one on the plane scan (BPRX_INDEX_QUEUE=0), and
    a second plane engine as the yardstick.  The forms differ only in the ranks equal items' occurrences get (the order LDS
    atomics arrive in), i.e. in the order k_item_seg sums an item's fp32 contributions: no bit equality is asked for.
    Bound, from the formats: an item here has at most ~80 occurrences (the two items every list holds) of at most
    lr * |g| * |row| <= 0.05 * 1 * 0.5 each; re-ordering an fp32 sum of c terms moves it by at most c * 2^-24 * sum|terms|
    = 80 * 6e-8 * 80 * 0.025 ~ 1e-5 in the worst case and by ~sqrt(c) * 2^-24 * |sum| ~ 1e-7 typically; three steps: atol 1e-6
    on the hot rows' scale is what two plane runs are held to as well.
    Measured on MI355X (max |difference| over Gu, Gi, Bi after three steps; the test prints both): plane vs plane 0 (at this size
    the scan's atomics arrived in the same order in both runs), queue vs plane 2.4e-7 (a few ulp of the hot rows)."""
    monkeypatch.setenv("BPRX_ITEM_MODE", "2")
    U, I, B = 300, 1000, 512
    lists = _lists(U, I, 5, seed=6, always=(7, I - 1))
    out = {}
    for name, pol in (("queue", "1"), ("plane", "0"), ("plane2", "0")):
        monkeypatch.setenv("BPRX_INDEX_QUEUE", pol)
        e, _, _ = _engine(U, I, B, seed=21)
        smp = _sampler("epoch", lists, I, e)
        for step in range(3):
            e.step(*smp.sample(B))
            assert e.lib.bprx_index_pass_queue(e.h) == int(pol), (name, step)
        e.sync_check()
        out[name] = {n: e.t[n].cpu().numpy().reshape(-1).copy() for n in ("Gu", "Gi", "Bi")}
    diff = lambda a, b: max(float(np.abs(out[a][n] - out[b][n]).max()) for n in ("Gu", "Gi", "Bi"))
    print("plane vs plane %.3g, queue vs plane %.3g" % (diff("plane", "plane2"), diff("queue", "plane")))
    assert diff("plane", "plane2") <= 1e-6
    assert diff("queue", "plane") <= 1e-6
