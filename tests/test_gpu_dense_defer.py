"""The deferred dense update: a bprx_step that is not asked for its loss leaves its dense E|Bp update to the next step's index pass
(the dense workgroups of k_index_seg), or to the first other call on the handle (bprx_settle_pending: the stand-alone kernel).
BPRX_DENSE_DEFER=0 keeps the stand-alone launch at the end of every step.

Every test builds two engines from the same seeded tables and feeds them the same batches, one under BPRX_DENSE_DEFER=0, and
compares with torch.equal: both forms run the same device function (dense_update_block) with the same tile -> block mapping, slab
order and order of the waves' sums, so they must leave the same bits -- in the tables, the Adam slots, the images (seen through
score_block) and the loss.

Shapes: U = 200, I = 1000, B = 1024 (segments from B = 500), k = 32.
  D = 256, d = 20  (PS 32)    bf16, fp8, fp32 x sgd, lazy adam, swept adam
  D = 384, d = 64  (PS 80)    bf16, sgd; fp8 at D = 512 (fp8 tables need D % 256 == 0: bprx_create rejects 384)
  D = 100, d = 64  (PS 80)    fp32, sgd: 13 tiles on 4 dense workgroups of four 256-thread sub-groups -- a partial last workgroup
                              (bf16 / fp8 tables have D % 128 == 0, so their tile count is always a multiple of four)
  D = 256, d = 256 (PS 272)   bf16, sgd: a tile of 544 threads' worth -- one 576-thread sub-group per dense workgroup
Batches.  Two handles agree bit for bit only if no sum of the step depends on an order the hardware picks (test_gpu_proj_mask's
docstring: segment ranks come from LDS atomics, and already two multiply-adds of one item's sum differ by their order; a user with
three run pieces takes three float atomics).  The plain batches are built for that: the users ascend, one run each, of a length and at an
offset that meet at most two workgroups of the triplet kernel (two commuting adds), every item is either used once, or is both the positive and the negative of the same triplet, twice over with the same
user (B = 1024 needs 2 048 occurrences from 1 000 items): there the score difference is exactly 0, g exactly -0.5, every
product exact and every partial sum of +-a, +-a an exact multiple of a, whatever the order.
The sampler's batches (EpochWalkSampler feeding the engine: byte planes, index pass kind 2) cannot be built that way: its
negatives are random, items repeat across the scanning waves and users across workgroups, and two runs of the SAME library
then differ in the last bits (measured on MI355X with BPRX_DENSE_DEFER=0 on BOTH sides, D = 256, d = 20: after two steps 138 /
840 / 192 of the 32 000 Gi values differ for bf16 sgd / fp32 sgd / fp8 lazy adam, max |diff| 7.5e-9 .. 1.9e-8, after six steps
461 / 4 798 / 536; the plain batches below: none, ever).  torch.equal between two handles is therefore not available there for any implementation; that test
checks the sequence exactly (kind 2 on every step, the pending state, updates carried and settled) and the tables at the
tolerances tests/test_gpu_step_plan.py uses for these very shapes, which come from fp32 summation order and the bf16 / e4m3
rounding of W and [E|Bp].  Bit equality of the two forms rests on the plain batches."""
import numpy as np
import pytest
import torch

import test_gpu_listmode as lm
from fashionvisualexpl_recommend_amd import _ffi
from fashionvisualexpl_recommend_amd.engine import EpochWalkSampler

pytestmark = pytest.mark.gpu

U, I, K, B = 200, 1000, 32, 1024
LR, REG = 0.05, 1e-3
ENV = {"BPRX_LIST_MODE": "1", "BPRX_ITEM_MODE": "1", "BPRX_PROJ_MASK": "1", "BPRX_SIDE_STREAM": "1", "BPRX_FWD_VARIANT": "4"}
BASE = [(256, 20, dt, opt) for dt in ("bf16", "fp8", "fp32") for opt in ("sgd", "lazy", "swept")]
SHAPES = BASE + [(384, 64, "bf16", "sgd"), (512, 64, "fp8", "sgd"), (100, 64, "fp32", "sgd"), (256, 256, "bf16", "sgd")]
IDS = ["D%d-d%d-%s-%s" % s for s in SHAPES]
_TABLES = {}


def _tables(D, d, dtype, seed=5):
    key = (D, d, dtype, seed)
    if key not in _TABLES:
        _TABLES[key] = lm._tables(U, I, K, d, D, seed=seed, dtype=dtype)
    return _TABLES[key]


def _engine(monkeypatch, defer, D, d, dtype, opt, tables=None):
    for n, v in ENV.items():
        monkeypatch.setenv(n, v)
    monkeypatch.delenv("BPRX_ADAM_LAZY", raising=False)
    monkeypatch.setenv("BPRX_DENSE_DEFER", "1" if defer else "0")
    e = lm._engine(model="vbpr", num_users=U, num_items=I, embed_k=K, embed_d=d, feat_dim=D, feat_dtype=dtype,
                   optimizer="sgd" if opt == "sgd" else "adam_tf23", lr=LR if opt == "sgd" else 0.01, reg=REG, max_batch=B,
                   adam_form={"sgd": None, "lazy": "lazy", "swept": "sweep"}[opt])
    return e.bind(**(tables or _tables(D, d, dtype)))


def _pair(monkeypatch, *shape):
    return _engine(monkeypatch, True, *shape), _engine(monkeypatch, False, *shape)


def _batch(seed, n=B):
    """n triplets whose step is the same bit for bit on every run (see the module docstring)."""
    rs = np.random.RandomState(seed)
    perm = rs.permutation(I)
    x = max(0, -(-(2 * n - I) // 3))                       # items that are positive and negative of two identical triplets
    y = 2 * (n - 2 * x)                                     # items used once, in y / 2 ordinary triplets
    assert x + y <= I and 2 * x + y // 2 == n
    pairs = [(it, it) for it in perm[:x]]
    singles = [(perm[x + 2 * q], perm[x + 2 * q + 1]) for q in range(y // 2)]
    # runs of equal users: 8 triplets at offsets that are multiples of 8, then 5 anywhere -- such a run meets at most two of the
    # triplet kernel's workgroups, whose triplet counts are multiples of 4 (four at d = 256); a small batch: one user per triplet
    if n <= U:
        lens = [1] * n
    else:
        nb5 = next(q for q in range(min(n // 5, U), -1, -1) if (n - 5 * q) % 8 == 0 and (n - 5 * q) // 8 + q <= U)
        lens = [8] * ((n - 5 * nb5) // 8) + [5] * nb5
    users = np.sort(rs.choice(U, size=len(lens), replace=False))
    u, i, j = [], [], []
    for usr, L in zip(users, lens):                         # identical triplets stay inside one run
        p = min(L // 2, len(pairs))
        take = [pairs.pop() for _ in range(p)] * 1
        for a, b in take:
            u += [usr] * 2; i += [a] * 2; j += [b] * 2
        for _ in range(L - 2 * p):
            a, b = singles.pop()
            u.append(usr); i.append(a); j.append(b)
    assert len(u) == n and not pairs and not singles
    return tuple(lm._dev(np.asarray(v, dtype=np.int32)) for v in (u, i, j))


def _lists(seed=3):
    rs = np.random.RandomState(seed)
    return [sorted(set(rs.randint(I, size=20).tolist())) for _ in range(U)]


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a + 0.0, b + 0.0), "%s: %d of %d values differ, max |diff| %.3g" % (
        what, int((a != b).sum()), a.numel(), float((a.double() - b.double()).abs().max()))


def _same_tables(ea, eb, what):
    ta, tb = ea.t, eb.t                                     # (the getter settles and syncs)
    for n in sorted(ta):
        if n != "F" and ta[n] is not None:
            _same(ta[n], tb[n], "%s: %s" % (what, n))


def _close(*engines):
    for e in engines:
        e.sync_check()
        e.close()


@pytest.mark.parametrize("D,d,dtype,opt", SHAPES, ids=IDS)
def test_six_steps_plain_batches(monkeypatch, D, d, dtype, opt):
    batches = [_batch(100 + s) for s in range(6)]
    # compared after every step: each deferred update is settled by the table getter (the stand-alone kernel, one step late)
    ea, eb = _pair(monkeypatch, D, d, dtype, opt)
    for s, b in enumerate(batches):
        ea.step(*b, want_loss=False); eb.step(*b, want_loss=False)
        assert ea.dense_pending() and not eb.dense_pending()
        _same_tables(ea, eb, "step %d" % s)
        assert not ea.dense_pending()
    _close(ea, eb)
    # compared at the end: five updates ride in the next step's index pass, the sixth is settled by score_block
    ea, eb = _pair(monkeypatch, D, d, dtype, opt)
    ea.profile(True)
    for b in batches:
        ea.step(*b, want_loss=False); eb.step(*b, want_loss=False)
    assert ea.dense_pending()
    prof = ea.profile_read()
    assert "dense_update" not in prof and prof["row_count"][1] == 6, prof
    _same(ea.score_block(0, U), eb.score_block(0, U), "score_block")
    assert not ea.dense_pending() and ea.profile_read()["dense_update"][1] == 1
    _same_tables(ea, eb, "after six steps")
    _close(ea, eb)


def _near_tables(ea, eb, dtype, opt, what):
    """the tolerances of tests/test_gpu_step_plan.py for these shapes (module docstring)"""
    lr = LR if opt == "sgd" else 0.01
    rt, at = (2e-5, 2e-6) if dtype == "fp32" else (2e-3, 1e-4)
    if opt != "sgd":
        at = max(at, 2e-3 * lr)
    of, oa = (0.0, 0.0) if dtype == "fp32" else ((1e-3, 3 * lr) if opt != "sgd" else (3e-2, 1e-2 * lr))
    ta, tb = ea.t, eb.t
    for n in ("Gu", "Gi", "Bi", "Tu", "E", "Bp"):
        lm._close(ta[n].cpu().numpy().reshape(-1), tb[n].cpu().numpy().reshape(-1), rt, at, "%s: %s" % (what, n), of, oa)


@pytest.mark.parametrize("D,d,dtype,opt", BASE, ids=IDS[:len(BASE)])
def test_six_steps_sampler_batches(monkeypatch, D, d, dtype, opt):
    ea, eb = _pair(monkeypatch, D, d, dtype, opt)
    sa, sb = (EpochWalkSampler(_lists(), I, seed=11).feeds(e) for e in (ea, eb))
    ea.profile(True)
    for s in range(6):
        ba, bb = sa.sample(B), sb.sample(B)
        for x, y in zip(ba, bb):
            assert torch.equal(x, y)
        ea.step(*ba, want_loss=False); eb.step(*bb, want_loss=False)
        assert ea.lib.bprx_index_pass_kind(ea.h) == 2 and eb.lib.bprx_index_pass_kind(eb.h) == 2     # the byte planes were used
        assert ea.dense_pending() and not eb.dense_pending()
        if s % 2:                                           # (odd steps: compared now, settled; even ones: carried by the next step)
            _near_tables(ea, eb, dtype, opt, "step %d" % s)
            assert not ea.dense_pending()
    prof = ea.profile_read()
    assert prof["dense_update"][1] == 3 and prof["row_count"][1] == 6, prof      # three settled by the getter, three carried
    sc_a, sc_b = ea.score_block(0, U), eb.score_block(0, U)
    assert float((sc_a - sc_b).abs().max()) <= 2e-3 * float(sc_b.abs().max()) + 1e-4
    _close(ea, eb)


def _mid_calls():
    small = _batch(900, 64)
    pairs = (lm._dev(np.arange(64, dtype=np.int32) % U), lm._dev(np.arange(64, dtype=np.int32) * 7 % I))
    Fnew = torch.as_tensor(lm._tables(U, 40, K, 20, 256, seed=77, dtype="bf16")["F"])

    def split(e):
        e.step_begin(*_batch(901))
        e.step_end(want_loss=False)

    # the entries behind the read gate that the Engine exposes: inputs that are the same for both engines
    g = torch.Generator().manual_seed(78)
    rnd = lambda *shape: torch.rand(shape, generator=g).cuda()
    rows = lm._dev(np.arange(64, dtype=np.int32) * 3 % 40)
    Pnew, Snew, Gu8, Tu8, S8 = rnd(40, 32), rnd(8, 40), rnd(8, K) - 0.5, rnd(8, 20) - 0.5, rnd(8, I)
    lists = _lists()
    from fashionvisualexpl_recommend_amd.models import draw_fold_pairs
    fold = draw_fold_pairs(lists[:8], I, 3, seed=1)

    def fold_in(e):
        Gu, Tu = torch.zeros((8, K), device="cuda"), torch.zeros((8, 20), device="cuda")
        return e.fold_in(*fold, 4, Gu, Tu, lr=0.05, reg=1e-3), Gu, Tu

    gated = {
        "feat_explain": lambda e: e.feat_explain(*pairs, 5, 256, maps=True),
        "feat_explain_new": lambda e: e.feat_explain_new(Fnew, pairs[0], rows, 5, 256),
        "score_new_block": lambda e: e.score_new_block(3, 50, Pnew),
        "score_rows_block": lambda e: e.score_rows_block(Gu8, Tu8, 0, 8),
        "fold_in": fold_in,
        "topk_rows": lambda e: e.topk_rows(Snew, 5),
        "topk_lists": lambda e: e.topk_lists(S8.clone(), e.csr(lists[:8]), 5),
        "eval_users": lambda e: e.eval_users(0, 8, S8.clone(), e.csr(lists), e.csr(lists[::-1]), 5),
        "eval_pos": lambda e: e.eval_pos(0, 8, S8, 0, I, e.csr(lists[::-1])),
        "sync_adam": lambda e: e.sync_adam(),
        "tables_dirty": lambda e: e.tables_dirty(),
        "set_adam_step": lambda e: setattr(e, "adam_step", e.adam_step),
        "clear_item_grad": lambda e: e.clear_item_grad(I),   # (the staging tables are all-zero between steps anyway)
        "clear_user_grad": lambda e: e.clear_user_grad(U),
        "sync_check": lambda e: e.sync_check(),
    }
    return {
        **gated,
        "score_pairs": lambda e: e.score_pairs(*pairs),
        "score_block": lambda e: e.score_block(3, 50),
        "step_project": lambda e: e.step_project(),
        "project_rows": lambda e: e.project_rows(Fnew),
        "list_step": lambda e: e.step(*small, want_loss=False),
        "split_step": split,
        "set_hyper": lambda e: e.set_hyper(0.02, 5e-3),         # the pending step keeps its own lr and reg
        "profile": lambda e: e.profile(True),
        "bind": lambda e: e.bind(**_tables(256, 20, "bf16", seed=6)),
    }


MID_CALLS = ("bind", "list_step", "profile", "project_rows", "score_block", "score_pairs", "set_hyper", "split_step", "step_project")
GATED_CALLS = ("clear_item_grad", "clear_user_grad", "eval_pos", "eval_users", "feat_explain", "feat_explain_new", "fold_in",
               "score_new_block", "score_rows_block", "set_adam_step", "sync_adam", "sync_check", "tables_dirty", "topk_lists", "topk_rows")


def _tensors(r):
    """the tensors of a call's result (a tensor, a dict or a tuple of them; anything else holds none), in a fixed order"""
    if isinstance(r, torch.Tensor):
        return [r]
    if isinstance(r, dict):
        return [r[n] for n in sorted(r)]
    return [t for x in r for t in _tensors(x)] if isinstance(r, (tuple, list)) else []


@pytest.mark.parametrize("call", MID_CALLS + GATED_CALLS)
def test_a_call_between_two_deferred_steps(monkeypatch, call):
    assert sorted(_mid_calls()) == sorted(MID_CALLS + GATED_CALLS)
    mid = _mid_calls()[call]
    ea, eb = _pair(monkeypatch, 256, 20, "bf16", "sgd")
    batches = [_batch(200 + s) for s in range(4)]
    first = (dict(ea.t), dict(eb.t))                        # (kept: a second bind replaces the engines' tables)
    for s, b in enumerate(batches):
        if s == 2:
            assert ea.dense_pending() and not eb.dense_pending()
            ra, rb = mid(ea), mid(eb)
            assert len(_tensors(ra)) == len(_tensors(rb))
            for q, (xa, xb) in enumerate(zip(_tensors(ra), _tensors(rb))):
                _same(xa, xb, "%s[%d]" % (call, q))
            # set_hyper and profile touch no table: the update stays pending and the next step carries it.  Every other call
            # settles first and leaves nothing pending (a list-mode step never defers its own update).
            assert ea.dense_pending() == (call in ("set_hyper", "profile")), call
        ea.step(*b, want_loss=False); eb.step(*b, want_loss=False)
    _same_tables(ea, eb, call)
    ea.settle()
    for n in ("E", "Bp", "Gi", "Tu"):                       # the tables of the first bind (a second bind settled on them first)
        _same(first[0][n], first[1][n], "%s: first %s" % (call, n))
    _same(ea.score_block(0, 8), eb.score_block(0, 8), call + ": score_block")
    _close(ea, eb)


def test_a_rejected_call_leaves_the_update_pending(monkeypatch):
    """A call turned away for its arguments, or by the gate for the handle's kind, launches nothing: the update stays pending and
    the next step carries it."""
    ea, eb = _pair(monkeypatch, 256, 20, "bf16", "sgd")
    u = lm._dev(np.arange(8, dtype=np.int32))
    S = torch.zeros((8, I), device="cuda")
    rejected = (lambda e: e.lib.bprx_score_block(e.h, 5, 3, S.data_ptr(), None), lambda e: e.topk(0, 8, S, e.csr(_lists()), 0),
                lambda e: e.feat_explain_new(torch.zeros((8, 256)), u, u, top=0), lambda e: e.lib.bprx_project_rows(e.h, None, 1 << 31, None, None),
                lambda e: e.explain_pairs(u, u))             # (the last: not a GradFashion handle)
    for s, call in enumerate(rejected):
        b = _batch(601 + s)
        ea.step(*b, want_loss=False); eb.step(*b, want_loss=False)
        assert ea.dense_pending() == 1
        ea.profile(True)
        for e in (ea, eb):
            try:
                rc = call(e)
            except _ffi.BprxError as err:
                rc = err.code
            assert rc == _ffi.E_INVALID, (s, rc)
        assert ea.dense_pending() == 1 and ea.profile_read() == {}, s
        b = _batch(650 + s)
        ea.step(*b, want_loss=False); eb.step(*b, want_loss=False)
        prof = ea.profile_read()
        assert "dense_update" not in prof and prof["row_count"][1] == 1, (s, prof)     # carried by the index pass
        ea.profile(False)
    _same_tables(ea, eb, "rejected calls")
    _close(ea, eb)


def test_an_empty_call_settles(monkeypatch):
    """A valid call with no work passes the gate like any other: nothing is pending afterwards."""
    ea, eb = _pair(monkeypatch, 256, 20, "bf16", "sgd")
    one = torch.zeros(64, device="cuda")
    p = one.data_ptr()
    empty = (lambda e: e.lib.bprx_score_pairs(e.h, None, None, 0, None, None), lambda e: e.lib.bprx_score_block(e.h, 7, 7, p, None),
             lambda e: e.lib.bprx_project_rows(e.h, None, 0, None, None),
             lambda e: e.lib.bprx_topk_lists(e.h, 0, None, None, None, 5, None, None, None, None),
             lambda e: e.lib.bprx_fold_in(e.h, p, None, None, 0, 1, 0.1, 0.0, 0, p, p, None, None))
    for s, call in enumerate(empty):
        b = _batch(700 + s)
        ea.step(*b, want_loss=False); eb.step(*b, want_loss=False)
        assert ea.dense_pending() == 1
        assert call(ea) == 0 and call(eb) == 0, s
        assert ea.dense_pending() == 0, s
    _same_tables(ea, eb, "empty calls")
    _close(ea, eb)


def test_borrowed_user_rows_leave_the_bound_ones_in_place(monkeypatch):
    """score_rows_block and ACF's score_block run the block-score kernels on other user rows than the bound Gu / Tu: what reads the
    bound rows scores the same bits before and after."""
    e = _engine(monkeypatch, True, 256, 20, "bf16", "sgd")
    g = torch.Generator().manual_seed(79)
    Gu8, Tu8 = (torch.rand((8, w), generator=g).cuda() - 0.5 for w in (K, 20))
    u, i = lm._dev(np.arange(64, dtype=np.int32) % U), lm._dev(np.arange(64, dtype=np.int32) * 7 % I)
    block, pairs = e.score_block(0, 8).clone(), e.score_pairs(u, i).clone()
    own = e.score_rows_block(e.t["Gu"], e.t["Tu"], 0, 8).clone()
    other = e.score_rows_block(Gu8, Tu8, 0, 8)
    _same(own, block, "the handle's own rows")
    assert not torch.equal(other, block)
    _same(e.score_block(0, 8), block, "score_block afterwards")
    _same(e.score_pairs(u, i), pairs, "score_pairs afterwards")
    _close(e)
    import test_gpu_acf as ta
    rs = np.random.RandomState(5)
    t = ta.random_tables(rs, 20, 50, 16, 64, 64, 64, scale=10.0)
    train = ta._lists(rs, 20, 50, rs.randint(1, 12, 20))
    a = ta._engine(t, ta._features(rs, 50, 9, 64, "fp32"), train, eval_lists=[x + [int(rs.randint(50))] for x in train])
    u, i = rs.randint(0, 20, 100), rs.randint(0, 50, 100)
    pairs, prof = a.score_pairs(u, i).clone(), a.acf_profiles(range(20)).clone()
    block = a.score_block(0, 20).clone()                    # (the block-score kernels on Gu' of the evaluation histories)
    _same(a.score_pairs(u, i), pairs, "ACF score_pairs afterwards")
    _same(a.acf_profiles(range(20)), prof, "ACF profiles afterwards")
    _same(a.score_block(0, 20), block, "ACF score_block again")
    _close(a)


def test_close_with_an_update_pending(monkeypatch):
    before = _ffi.lib().bprx_live_device_allocs()
    e = _engine(monkeypatch, True, 256, 20, "bf16", "sgd")
    e.step(*_batch(300), want_loss=False)
    assert e.dense_pending()
    torch.cuda.synchronize()
    e.close()                                               # dropped, not launched: the tables are the caller's again
    torch.cuda.synchronize()
    assert _ffi.lib().bprx_live_device_allocs() == before


@pytest.mark.parametrize("dtype,opt", [("bf16", "sgd"), ("fp8", "lazy"), ("fp32", "swept")])
def test_loss_lag_gives_the_same_losses(monkeypatch, dtype, opt):
    ea, eb = _pair(monkeypatch, 256, 20, dtype, opt)
    la, lb = (torch.zeros(6, dtype=torch.float32, device="cuda") for _ in range(2))
    ea.set_loss_lag(True)
    for s in range(6):
        b = _batch(400 + s)
        ea.step(*b, loss_out=la, loss_index=s); eb.step(*b, loss_out=lb, loss_index=s)
        assert ea.dense_pending() and not eb.dense_pending()
    ea.settle()                                             # the sixth loss lands behind the settling launch
    torch.cuda.synchronize()
    assert float(lb.abs().min()) > 0.0
    _same(la, lb, "losses")
    _same_tables(ea, eb, "loss lag")
    # without the lag a step that is asked for its loss keeps the parent's sequence
    ea.set_loss_lag(False)
    ea.step(*_batch(410), loss_out=la, loss_index=0)
    assert not ea.dense_pending()
    _close(ea, eb)


def test_profiler_counts_and_pending_state(monkeypatch):
    e = _engine(monkeypatch, True, 256, 20, "bf16", "sgd")
    e.profile(True)
    assert not e.dense_pending()
    for s in range(3):
        e.step(*_batch(500 + s), want_loss=False)
        prof = e.profile_read()
        assert "dense_update" not in prof and prof["row_count"][1] == 1 and "loss_reduce" not in prof, (s, prof)
        assert e.dense_pending()
    e.settle()
    prof = e.profile_read()
    assert prof["dense_update"][1] == 1 and len(prof) == 1, prof
    assert not e.dense_pending()
    e.settle()                                              # nothing pending: returns at once, launches nothing
    assert e.profile_read() == {}
    e.step(*_batch(510))                                    # asked for its loss: today's sequence
    prof = e.profile_read()
    assert prof["dense_update"][1] == 1 and prof["loss_reduce"][1] == 1 and not e.dense_pending(), prof
    _close(e)
