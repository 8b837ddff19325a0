"""Folding in users the model was not trained on, on the MI355X, against the float64 restatement (tests/fold_in_ref.py):
bprx_fold_in, bprx_score_rows_block, bprx_topk_lists and the model methods on top of them.

Allowance per compared output (the project's rule, tests/test_gpu_new_items.py): 32 x the max-abs deviation of the FLOAT32
restatement from the float64 one over the case, never below one float32 ulp of the output's largest magnitude.  Every check prints
its triple (float32 deviation / allowance / GPU deviation).  What is exact is checked exactly: two calls, a user's row wherever it
stands and whatever n is, the cached against the re-gathering form, the score and top-K calls against their user-id twins.

Inputs: I = 300, tables ~ N(0, 0.3) (P = F.[E|Bp] with E scaled so that P is), start rows ~ N(0, 0.3).  130 users with 0, 1, 3, 4, 5,
17, 64, 65, 200 and 1..40 random pairs (a duplicated pair and an i == j pair among them) and one user with 3 000 pairs, past any
LDS share.  That user's pairs set its 30 best against its 30 worst items under its start row: 3 000 RANDOM pairs have a summed
curvature of about 0.25 x 3 000 x 0.18 = 135 per direction, so plain sgd at lr = 0.02 oscillates on them in exact arithmetic
(lr x curvature = 2.7 > 2) and loss_20 < loss_1 would not hold for the definition itself; a consistent history (sigmoid(-x) small)
keeps the curvature far below 2 / lr.  On the CPU the float64 restatement's loss falls for every user with pairs at every width
for seeds 0, 1, 2, the float32 rows deviate by 3e-7 .. 1e-6, and Adam's left-out share is 0.6 .. 1.6 %."""
import gc
from argparse import Namespace

import numpy as np
import pytest
import torch

import fold_in_ref as R
from fashionvisualexpl_recommend_amd import _ffi, synth
from test_gpu_feat_explain import _bits, _snapshot, _tables, _unique_batches, _vbpr

pytestmark = pytest.mark.gpu

I = 300
WIDTHS = [(5, 0), (16, 12), (64, 64), (128, 20), (200, 271)]
BIG = 9                                                      # the user with 3 000 pairs
SGD = dict(steps=20, lr=0.02, reg=1e-3, optimizer="sgd")
ADAM = dict(steps=3, lr=0.05, reg=1e-3, optimizer="adam_tf23")


def _allow(r64, r32):
    dev = float(np.abs(r64 - r32.astype(np.float64)).max())
    return dev, max(32.0 * dev, float(np.spacing(np.float32(np.abs(r64).max()))))


def _report(tag, r64, r32, got):
    dev, allow = _allow(r64, r32)
    gdev = float(np.abs(got.astype(np.float64) - r64).max())
    print("%s: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (tag, dev, allow, gdev))
    return gdev, allow


def _item_tables(k, d, U=8, D=32, seed=0):
    rs = np.random.RandomState(seed)
    n = lambda *s: (rs.standard_normal(s) * 0.3).astype(np.float32)
    t = dict(Gu=n(U, k), Gi=n(I, k), Bi=n(I))
    if d:
        F = np.abs(rs.standard_normal((I, D))).astype(np.float32)
        F /= F.max()
        scale = 1.0 / np.sqrt((F.astype(np.float64) ** 2).sum(1).mean())
        t.update(Tu=n(U, d), F=F, E=(n(D, d) * scale).astype(np.float32), Bp=(n(D) * scale).astype(np.float32))
    return t


def _engine(t, optimizer="sgd", B=64, **kw):
    from fashionvisualexpl_recommend_amd.engine import Engine
    U, k = t["Gu"].shape
    if "F" not in t:
        return Engine(model="bprmf", num_users=U, num_items=I, embed_k=k, optimizer=optimizer, lr=0.05, reg=1e-3, max_batch=B,
                      **kw).bind(t["Gu"], t["Gi"], t["Bi"])
    D, d = t["E"].shape
    return Engine(model="vbpr", num_users=U, num_items=I, embed_k=k, embed_d=d, feat_dim=D, feat_dtype="fp32", optimizer=optimizer,
                  lr=0.05, reg=1e-3, max_batch=B, **kw).bind(**t)


def _proj(e, t):
    """The item projections the handle holds (fp32 features: project_rows runs the catalogue's kernels on the bound table)."""
    return e.project_rows(t["F"]).cpu().numpy()[:, :e.d + 1] if e.d else None


def _users(t, P, k, d, seed):
    """(ptr, pos, neg, W0) of the 130 new users of the module docstring."""
    rs = np.random.RandomState(seed + 100)
    counts = [0, 1, 3, 4, 5, 17, 64, 65, 200] + list(rs.randint(1, 41, size=121))
    W0 = (rs.standard_normal((len(counts), k + d)) * 0.3).astype(np.float32)
    pos = [rs.randint(I, size=c) for c in counts]
    neg = [rs.randint(I, size=c) for c in counts]
    Z = np.concatenate([t["Gi"], P[:, :d]], 1) if d else t["Gi"]
    c = t["Bi"] + (P[:, d] if d else 0)
    order = np.argsort(Z.astype(np.float64) @ W0[BIG].astype(np.float64) + c)
    counts[BIG] = 3000
    pos[BIG], neg[BIG] = order[-30:][rs.randint(30, size=3000)], order[:30][rs.randint(30, size=3000)]
    pos[7][3], neg[7][3] = pos[7][2], neg[7][2]              # a pair twice
    neg[6][5] = pos[6][5]                                     # i == j
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return ptr, np.concatenate(pos).astype(np.int32), np.concatenate(neg).astype(np.int32), W0


def _fold(e, ptr, pos, neg, W0, **hp):
    """One bprx_fold_in call from the start rows W0: (Gu, Tu or None, loss) as numpy arrays."""
    k, d = e.k, e.d
    Gu = torch.as_tensor(np.ascontiguousarray(W0[:, :k]), device="cuda")
    Tu = torch.as_tensor(np.ascontiguousarray(W0[:, k:]), device="cuda") if d else None
    loss = e.fold_in(ptr, pos, neg, hp["steps"], Gu, Tu, lr=hp["lr"], reg=hp["reg"], optimizer=hp["optimizer"])
    return Gu.cpu().numpy(), (Tu.cpu().numpy() if d else None), loss.cpu().numpy()


def _sub(ptr, pos, neg, W0, users):
    """The call for the listed users only, in the listed order."""
    users = list(users)
    cnt = [int(ptr[u + 1] - ptr[u]) for u in users]
    p = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    take = np.concatenate([np.arange(ptr[u], ptr[u + 1]) for u in users] + [np.zeros(0, np.int64)]).astype(np.int64)
    return p, pos[take], neg[take], W0[users]


_cache = {}


def _case(k, d):
    """Tables, engine, users, both restatements (sgd, adam) and the GPU's n = 130 results of one width: made once, never changed."""
    if (k, d) not in _cache:
        t = _item_tables(k, d, seed=k)
        e = _engine(t)
        P = _proj(e, t)
        ptr, pos, neg, W0 = _users(t, P, k, d, seed=k)
        c = dict(t=t, e=e, P=P, ptr=ptr, pos=pos, neg=neg, W0=W0)
        G0, T0 = W0[:, :k], (W0[:, k:] if d else None)
        for name, hp in (("sgd", SGD), ("adam", ADAM)):
            c[name + "64"], c[name + "32"] = (R.fold_in(t["Gi"], t["Bi"], P, ptr, pos, neg, G0, T0, hp["steps"], hp["lr"], hp["reg"],
                                                        hp["optimizer"], dt) for dt in (np.float64, np.float32))
            c[name + "_gpu"] = _fold(e, ptr, pos, neg, W0, **hp)
        e.sync_check()
        _cache[(k, d)] = c
    return _cache[(k, d)]


def _rows(res, d):
    """[n, k + d] from a restatement dict or a (Gu, Tu, loss) triple."""
    Gu, Tu = (res["Gu"], res["Tu"]) if isinstance(res, dict) else res[:2]
    return np.concatenate([Gu, Tu], 1) if d else Gu


# ---- against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", WIDTHS)
def test_sgd_rows_and_loss_against_float64(k, d):
    c = _case(k, d)
    r64, r32, got = c["sgd64"], c["sgd32"], c["sgd_gpu"]
    gdev, allow = _report("sgd rows k=%d d=%d" % (k, d), _rows(r64, d), _rows(r32, d), _rows(got, d))
    assert gdev <= allow
    ldev, lallow = _report("sgd loss_20 k=%d d=%d" % (k, d), r64["loss"], r32["loss"], got[2])
    assert ldev <= lallow
    first = _fold(c["e"], c["ptr"], c["pos"], c["neg"], c["W0"], **dict(SGD, steps=1))[2]
    fdev, fallow = _report("sgd loss_1 k=%d d=%d" % (k, d), r64["loss_first"], r32["loss_first"], first)
    assert fdev <= fallow
    has = np.diff(c["ptr"]) > 0
    assert (r64["loss"][has] < r64["loss_first"][has]).all()                      # the definition itself, on these inputs
    assert (got[2][has] < first[has]).all(), np.nonzero(~(got[2] < first) & has)[0]
    assert got[2][0] == 0 and np.array_equal(_bits(_rows(got, d)[0]), _bits(c["W0"][0]))    # no pairs: the row stays, loss 0


@pytest.mark.parametrize("k,d", WIDTHS)
def test_adam_rows_against_float64(k, d):
    """Adam's first steps turn the sign of a near-zero gradient into a +-lr move: entries (user, element) whose float64 |g| at any
    step is below 1e-3 of that user's largest |g| at that step are left out; at most 2 % of them may be."""
    c = _case(k, d)
    r64, r32, got = c["adam64"], c["adam32"], c["adam_gpu"]
    has = np.diff(c["ptr"]) > 0
    keep = np.ones((len(has), k + d), bool)
    for r in np.nonzero(has)[0]:
        g = np.abs(r64["grads"][r])
        keep[r] = ~(g < 1e-3 * g.max(1, keepdims=True)).any(0)
    share = 1.0 - keep[has].mean()
    print("adam k=%d d=%d: left-out share %.4f" % (k, d, share))
    assert share <= 0.02
    a, b, g = _rows(r64, d), _rows(r32, d), _rows(got, d)
    gdev, allow = _report("adam rows k=%d d=%d" % (k, d), a[keep], b[keep], g[keep])
    assert gdev <= allow
    ldev, lallow = _report("adam loss_3 k=%d d=%d" % (k, d), r64["loss"], r32["loss"], got[2])
    assert ldev <= lallow


@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
@pytest.mark.parametrize("k,d", [(5, 0), (16, 12), (64, 64)])
def test_one_step_moves_a_trained_users_row_as_bprx_step_does(k, d, opt):
    """T = 1 from a trained user's rows against the engine's own step on that user's pairs (adam_tf23 at adam_step = 0)."""
    t = _item_tables(k, d, seed=40 + k)
    e = _engine(t, optimizer=opt)
    P = _proj(e, t)
    rs = np.random.RandomState(41)
    u, B, lr, reg = 5, 37, 0.05, 1e-3
    pos, neg = rs.randint(I, size=B).astype(np.int32), rs.randint(I, size=B).astype(np.int32)
    pos[3], neg[3] = pos[2], neg[2]
    neg[7] = pos[7]
    W0 = np.concatenate([t["Gu"][u:u + 1], t["Tu"][u:u + 1]], 1) if d else t["Gu"][u:u + 1]
    hp = dict(steps=1, lr=lr, reg=reg, optimizer=opt)
    fold = _rows(_fold(e, [0, B], pos, neg, W0, **hp), d)[0]
    r64, r32 = (_rows(R.fold_in(t["Gi"], t["Bi"], P, [0, B], pos, neg, W0[:, :k], W0[:, k:] if d else None, 1, lr, reg, opt, dt), d)[0]
                for dt in (np.float64, np.float32))
    assert e.adam_step == 0
    dev = lambda x: torch.as_tensor(x, device="cuda")
    e.step(dev(np.full(B, u, np.int32)), dev(pos), dev(neg))
    stepped = torch.cat([e.t["Gu"][u], e.t["Tu"][u]]).cpu().numpy() if d else e.t["Gu"][u].cpu().numpy()
    _, allow = _allow(r64, r32)
    gap = float(np.abs(stepped.astype(np.float64) - fold).max())
    print("T=1 %s k=%d d=%d: allowance %.3e / fold_in - float64 %.3e / bprx_step - float64 %.3e / bprx_step - fold_in %.3e" % (
        opt, k, d, allow, np.abs(fold - r64).max(), np.abs(stepped - r64).max(), gap))
    assert np.abs(stepped - W0[0]).max() > 1e-3                                   # (the step moved the row)
    assert gap <= allow
    e.sync_check()
    e.close()


# ---- bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", WIDTHS)
def test_a_users_bits_depend_on_nothing_but_the_user(monkeypatch, k, d):
    c = _case(k, d)
    e, ptr, pos, neg, W0 = c["e"], c["ptr"], c["pos"], c["neg"], c["W0"]
    for name, hp in (("sgd", SGD), ("adam", ADAM)):
        full = c[name + "_gpu"]
        rows, loss = _rows(full, d), full[2]
        again = _fold(e, ptr, pos, neg, W0, **hp)
        assert np.array_equal(_bits(rows), _bits(_rows(again, d))) and np.array_equal(_bits(loss), _bits(again[2])), "two calls"
        perm = np.random.RandomState(7).permutation(len(W0))
        shuffled = _fold(e, *_sub(ptr, pos, neg, W0, perm), **hp)
        assert np.array_equal(_bits(_rows(shuffled, d)), _bits(rows[perm])) and np.array_equal(_bits(shuffled[2]), _bits(loss[perm]))
        for users in ([0], [1], [5], [BIG], [8], [129], range(4), range(5)):      # n = 1, 4, 5
            users = list(users)
            part = _fold(e, *_sub(ptr, pos, neg, W0, users), **hp)
            assert np.array_equal(_bits(_rows(part, d)), _bits(rows[users])), (name, users)
            assert np.array_equal(_bits(part[2]), _bits(loss[users])), (name, users)
    monkeypatch.setenv("BPRX_FOLD_CACHE", "0")                                    # read at create: every user re-gathers per step
    e0 = _engine(c["t"])
    for name, hp in (("sgd", SGD), ("adam", ADAM)):
        plain = _fold(e0, ptr, pos, neg, W0, **hp)
        assert np.array_equal(_bits(_rows(plain, d)), _bits(_rows(c[name + "_gpu"], d))), name
        assert np.array_equal(_bits(plain[2]), _bits(c[name + "_gpu"][2])), name
    e0.sync_check()
    e0.close()


# ---- neutrality and lifecycle ----------------------------------------------------------------------------------------------------
def _new_user_calls(e, seed=60):
    """fold_in, score_rows_block and topk_lists for 20 new users of a 600-item engine."""
    rs = np.random.RandomState(seed)
    hist = [list(rs.choice(600, size=rs.randint(1, 9), replace=False)) for _ in range(20)]
    from fashionvisualexpl_recommend_amd.models import draw_fold_pairs
    ptr, pos, neg = draw_fold_pairs(hist, 600, 3, seed=1)
    Gu = torch.zeros((20, e.k), device="cuda")
    Tu = torch.zeros((20, e.d), device="cuda")
    e.fold_in(ptr, pos, neg, 4, Gu, Tu, lr=0.05, reg=1e-3)
    sc = e.score_rows_block(Gu, Tu, 0, 20)
    return e.topk_lists(sc, e.csr(hist), 10)


@pytest.mark.parametrize("opt,form", [("sgd", None), ("adam_tf23", "lazy"), ("adam_tf23", "sweep")])
def test_the_calls_leave_the_state_alone(monkeypatch, opt, form):
    """Tables and Adam slots are bit-identical before and after the three calls, and a 6-step run with them between steps 3 and 4
    ends bit-identical to a run without them (duplicate-free batches: the step itself is then free of atomic-order noise)."""
    t = _tables(300, 600, 16, 12, 128, 100, "bf16", seed=17)
    batches = _unique_batches(300, 600, 64, 6, seed=18)
    end = []
    if form is not None:
        monkeypatch.setenv("BPRX_ADAM_LAZY", "1" if form == "lazy" else "0")
    for with_calls in (False, True):
        e = _vbpr(t, "bf16", optimizer=opt, B=64)
        if form is not None:
            assert e.adam_is_lazy() == (form == "lazy")
        for s, b in enumerate(batches):
            if s == 3 and with_calls:
                e.sync_adam()
                before = _snapshot(e)
                live = e.lib.bprx_live_device_allocs()
                _new_user_calls(e)
                torch.cuda.synchronize()
                assert e.lib.bprx_live_device_allocs() == live
                after = _snapshot(e)
                for n in before:
                    assert torch.equal(before[n].view(torch.int32), after[n].view(torch.int32)), n
            e.step(*b)
        e.sync_check()
        end.append({n: v.cpu().numpy() for n, v in e.t.items() if n != "F"})
        e.close()
    for n in end[0]:
        assert np.array_equal(_bits(end[0][n]), _bits(end[1][n])), "%s: %d words differ" % (
            n, int((_bits(end[0][n]) != _bits(end[1][n])).sum()))


def test_errors_leave_the_handle_usable_and_no_allocation_behind():
    from fashionvisualexpl_recommend_amd.engine import Engine
    from acf_ref import random_tables
    from test_gpu_acf import _engine as _acf_engine, _features as _acf_features, _lists as _acf_lists
    lib = _ffi.lib()
    gc.collect()
    live = lib.bprx_live_device_allocs()
    t = _item_tables(16, 12, seed=70)
    e = _engine(t)
    wide = Engine(model="bprmf", num_users=2, num_items=4, embed_k=1025, optimizer="sgd", max_batch=8)
    wide.bind(np.zeros((2, 1025), np.float32), np.zeros((4, 1025), np.float32), np.zeros(4, np.float32))
    unbound = Engine(model="bprmf", num_users=8, num_items=I, embed_k=16, optimizer="sgd", max_batch=8)
    rs = np.random.RandomState(71)
    acf = _acf_engine(random_tables(rs, 6, 20, 16, 8, 4, 4), _acf_features(rs, 20, 2, 8, "fp32"), _acf_lists(rs, 6, 20, [2, 0, 3, 1, 2, 2]))
    held = lib.bprx_live_device_allocs()
    ptr = torch.as_tensor(np.array([0, 2, 3], np.int64), device="cuda")
    pos = torch.as_tensor(np.array([1, 2, 3], np.int32), device="cuda")
    neg = torch.as_tensor(np.array([4, 5, 6], np.int32), device="cuda")
    Gu, Tu, loss = torch.zeros((2, 16), device="cuda"), torch.zeros((2, 12), device="cuda"), torch.zeros(2, device="cuda")
    p = lambda x: None if x is None else x.data_ptr()

    def call(h, n=2, steps=1, opt=0, ptr_=ptr, pos_=pos, neg_=neg, Gu_=Gu, Tu_=Tu):
        return lib.bprx_fold_in(h, p(ptr_), p(pos_), p(neg_), n, steps, 0.05, 1e-3, opt, p(Gu_), p(Tu_), p(loss), None)

    assert call(e.h) == 0
    good = Gu.cpu().numpy().copy()
    assert np.abs(good).max() > 0
    assert call(e.h, n=0) == 0 and call(e.h, n=0, pos_=None, neg_=None) == 0
    for kw in (dict(n=-1), dict(steps=0), dict(opt=2), dict(ptr_=None), dict(pos_=None), dict(neg_=None), dict(Gu_=None),
               dict(Tu_=None)):
        assert call(e.h, **kw) == _ffi.E_INVALID, kw
    assert call(acf.h, Tu_=None) == _ffi.E_INVALID
    G1025 = torch.zeros((2, 1025), device="cuda")
    assert call(wide.h, Gu_=G1025, Tu_=None) == _ffi.E_INVALID and "1024" in lib.bprx_last_error(wide.h).decode()
    assert call(unbound.h, Tu_=None) == _ffi.E_STATE
    sc = torch.zeros((2, I), device="cuda")
    rows = lambda h, G=Gu, T=Tu, n=2, r0=0, r1=2, out=sc: lib.bprx_score_rows_block(h, p(G), p(T), n, r0, r1, p(out), None)
    assert rows(e.h) == 0 and rows(e.h, r0=1, r1=1, G=None, T=None, out=None) == 0
    for kw in (dict(n=-1), dict(r0=-1), dict(r1=3), dict(r0=2, r1=1), dict(G=None), dict(T=None), dict(out=None)):
        assert rows(e.h, **kw) == _ffi.E_INVALID, kw
    assert rows(acf.h, T=None) == _ffi.E_INVALID and rows(unbound.h, T=None) == _ffi.E_STATE
    lp, li = torch.as_tensor(np.array([0, 1, 1], np.int64), device="cuda"), torch.as_tensor(np.array([3], np.int32), device="cuda")
    idx, val, flag = torch.zeros((2, 5), dtype=torch.int32, device="cuda"), torch.zeros((2, 5), device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    topk = lambda n=2, K=5, s=sc, a=lp, b=li: lib.bprx_topk_lists(e.h, n, p(s), p(a), p(b), K, p(idx), p(val), p(flag), None)
    assert topk() == 0 and topk(n=0) == 0
    for kw in (dict(n=-1), dict(K=0), dict(K=1025), dict(s=None), dict(a=None), dict(b=None)):
        assert topk(**kw) == _ffi.E_INVALID, kw
    e.sync_check()
    # item ids out of range: clamped, and reported by sync_check (once); the handle goes on working
    bad = torch.as_tensor(np.array([1, I, 3], np.int32), device="cuda")
    Gu.zero_(); Tu.zero_()
    assert call(e.h, pos_=bad) == 0
    with pytest.raises(_ffi.BprxError) as err:
        e.sync_check()
    assert err.value.code == _ffi.E_RANGE
    clamped = Gu.cpu().numpy().copy()
    Gu.zero_(); Tu.zero_()
    assert call(e.h, pos_=torch.as_tensor(np.array([1, I - 1, 3], np.int32), device="cuda")) == 0
    assert np.array_equal(_bits(clamped), _bits(Gu.cpu().numpy()))
    Gu.zero_(); Tu.zero_()
    assert call(e.h) == 0 and np.array_equal(_bits(good), _bits(Gu.cpu().numpy()))
    e.sync_check()
    assert lib.bprx_live_device_allocs() == held                    # the calls allocated nothing
    for eng in (e, wide, unbound, acf):
        eng.close()
    assert lib.bprx_live_device_allocs() == live


# ---- scores and lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", [(16, 12), (15, 12), (16, 0), (5, 0)])
def test_score_rows_block_is_score_block_for_the_handles_own_rows(k, d):
    """A slice of the handle's own Gu / Tu: the bits of score_block, with the matrix unit (even k and d) and without."""
    t = _item_tables(k, d, U=300, seed=80 + k)
    e = _engine(t)
    for u0, u1 in ((0, 300), (7, 8), (120, 259)):
        want = e.score_block(u0, u1).cpu().numpy()
        Gu = e.t["Gu"][u0:u1].contiguous()
        Tu = e.t["Tu"][u0:u1].contiguous() if d else None
        got = e.score_rows_block(Gu, Tu, 0, u1 - u0).cpu().numpy()
        assert np.array_equal(_bits(want), _bits(got)), (u0, u1)
        inner = e.score_rows_block(e.t["Gu"], e.t["Tu"] if d else None, u0, u1).cpu().numpy()      # a row range of a larger table
        assert np.array_equal(_bits(want), _bits(inner)), (u0, u1)
    e.sync_check()
    e.close()


@pytest.mark.parametrize("K", [1, 20, 300, 400])
def test_topk_lists_is_topk_with_the_lists_rebased(K):
    """The training CSR of users [u0, u1) re-based to row 0: bprx_topk's lists, values and flags bit for bit (ties inside the list,
    at its boundary and K > I among them)."""
    t = _item_tables(16, 0, U=130, seed=90)
    e = _engine(t)
    tr, _, _ = synth.make_interactions(130, I, per_user=8, seed=91)
    csr = e.csr(tr)
    for u0, u1 in ((0, 130), (40, 77)):
        S = e.score_block(u0, u1)
        S[:, 11] = S[:, 5]                                           # equal scores in every row
        S2 = S.clone()
        want = e.topk(u0, u1, S, csr, K)
        got = e.topk_lists(S2, e.csr(tr[u0:u1]), K)
        for a, b, n in zip(want, got, ("idx", "val", "flag")):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())), (n, u0, u1)
        assert torch.equal(S.view(torch.int32), S2.view(torch.int32))        # the same items masked in place
        assert want[2].any() or K == 1
    e.sync_check()
    e.close()


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _model(rec, U=130, Inum=60, **kw):
    from fashionvisualexpl_recommend_amd.models import BPRMF, VBPR
    p = dict(dataset="vb", validation=True, batch_size=64, epochs=1, batch_eval=128, embed_k=8, embed_d=6, lr=0.05, reg=1e-3,
             top_k=10, verbose=-1, restore_epochs=1, rec=rec, best_metric="ndcg", optimizer="sgd", init_seed=5, dtype="fp32")
    p.update(kw)
    p = Namespace(**p)
    tr, va, te = synth.make_interactions(U, Inum, per_user=8, seed=39)
    data = Namespace(num_users=U, num_items=Inum, training_list=tr, validation_list=va, test_list=te, params=p)
    if rec == "bprmf":
        return BPRMF(data, p), tr
    return VBPR(data, p, features=synth.make_features(Inum, 32, seed=40) * 3.7), tr


@pytest.mark.parametrize("rec", ["bprmf", "vbpr"])
def test_recommend_new_users_ranks_as_the_float64_restatement(rec):
    """End to end on synth: fold_in_users -> score_rows_block -> topk_lists against the restatement's ranking, for the rows the GPU
    did not flag, wherever the score allowance rules out a near-tie around a list position."""
    from fashionvisualexpl_recommend_amd.models import draw_fold_pairs
    m, tr = _model(rec)
    eng, Inum, K = m.engine, 60, 10
    hist = [list(h) for h in tr[:40]] + [[], list(range(Inum))]     # the training lists of 40 users, a user without history, one with all
    fold = dict(steps=12, negatives=3, seed=3)
    idx, val = m.recommend_new_users(hist, **fold)
    assert idx.shape == val.shape == (42, K)
    Gu, Tu = m.fold_in_users(hist, **fold)
    assert (Tu is None) == (rec == "bprmf") and not Gu[40].any() and not Gu[41].any()    # no pairs: the zero start row stays
    ptr, pos, neg = draw_fold_pairs(hist, Inum, 3, seed=3)
    P = eng.project_rows(eng.t["F"]).cpu().numpy()[:, :eng.d + 1] if eng.d else None
    Gi, Bi = eng.t["Gi"].cpu().numpy(), eng.t["Bi"].cpu().numpy()
    z = lambda w: np.zeros((42, w), np.float32)
    r64, r32 = (R.fold_in(Gi, Bi, P, ptr, pos, neg, z(eng.k), z(eng.d) if eng.d else None, 12, 0.05, 1e-3, "sgd", dt)
                for dt in (np.float64, np.float32))
    gdev, allow = _report("model rows %s" % rec, _rows(r64, eng.d), _rows(r32, eng.d), _rows((Gu.cpu().numpy(), Tu.cpu().numpy() if eng.d else None), eng.d))
    assert gdev <= allow
    S64 = R.scores(Gi, Bi, P, r64["Gu"], r64["Tu"])
    S32 = R.scores(Gi, Bi, P, r32["Gu"], r32["Tu"], np.float32)
    _, sallow = _allow(S64, S32)
    sc = eng.score_rows_block(Gu, Tu, 0, 42)
    assert float(np.abs(sc.cpu().numpy() - S64).max()) <= sallow
    flag = eng.topk_lists(sc.clone(), eng.csr(hist), K)[2].cpu().numpy()
    checked = 0
    for r in range(41):                                              # (row 41 masks every item: flagged)
        row = S64[r].copy()
        row[hist[r]] = -np.inf
        order = np.argsort(-row, kind="stable")
        gaps = row[order[:K]] - row[order[1:K + 1]]
        if flag[r] or (gaps <= 2 * sallow).any():
            continue
        assert np.array_equal(idx[r], order[:K]), r
        assert np.abs(val[r] - row[order[:K]]).max() <= sallow
        assert not set(idx[r].tolist()) & set(hist[r])
        checked += 1
    print("model %s: %d of 41 rows ranked as float64" % (rec, checked))
    assert checked >= 20 and flag[41] == 1
    eng.sync_check()
    eng.close()


# ---- files -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", ["bprmf", "vbpr"])
def test_cli_writes_new_user_files_next_to_unchanged_recommendations(tmp_path, rec):
    import os
    from fashionvisualexpl_recommend_amd import train_rec
    U, Inum, top_k = 30, 60, 10
    tr, va, te = synth.make_interactions(U, Inum, per_user=8, seed=53)
    synth.write_dataset(str(tmp_path), "toy", tr, va, te, Inum, features=synth.make_features(Inum, 32, seed=55) if rec == "vbpr" else None)
    hist = {"new shopper": [3, 9, 40], "b": [7], "c 3": [5, 6, 5]}
    rows = [("new shopper", 3), ("b", 7), ("new shopper", 9), ("c 3", 5), ("c 3", 6), ("new shopper", 40), ("c 3", 5)]
    (tmp_path / "new.tsv").write_text("".join("%s\t%d\n" % r for r in rows))
    # --batch_size 1: a step adds at most one term to a gradient row, so runs of the same seed agree bit for bit
    common = ["--rec", rec, "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--reg", "0.01", "--top_k", str(top_k), "--lr", "0.01", "--optimizer", "sgd"]
    res = [str(tmp_path / ("res%d" % q)) for q in range(2)]
    train_rec.train(common + ["--results_root", res[0]])
    train_rec.train(common + ["--results_root", res[1], "--new_users", str(tmp_path / "new.tsv"), "--fold_steps", "9", "--fold_negatives", "3"])
    rdir = [os.path.join(r, "rec_results", "toy", rec) for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] if "new-user-" in f]
    assert [f for f in files[1] if "new-user-" not in f] == files[0]
    base = [f for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(base) == 2
    for f in base:                                                   # the catalogue's files: the bytes of the run without the flag
        assert open(os.path.join(rdir[0], f), "rb").read() == open(os.path.join(rdir[1], f), "rb").read(), f
        new = f.replace("recs-", "new-user-recs-", 1)
        assert new in files[1]
        got = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], new))]
        assert len(got) == 3 * top_k and all(len(r) == 3 for r in got)
        assert [r[0] for r in got] == [lab for lab in ("new shopper", "b", "c 3") for _ in range(top_k)]     # first-appearance order
        for q, lab in enumerate(("new shopper", "b", "c 3")):
            blk = got[q * top_k:(q + 1) * top_k]
            sc = [float(r[2]) for r in blk]
            assert sc == sorted(sc, reverse=True) and len({r[1] for r in blk}) == top_k
            assert all(0 <= int(r[1]) < Inum for r in blk) and not {int(r[1]) for r in blk} & set(hist[lab])
