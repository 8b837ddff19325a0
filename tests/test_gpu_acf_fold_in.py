"""Folding new users into ACF on the MI355X, against the float64 restatement (tests/acf_fold_in_ref.py): bprx_acf_fold_in,
bprx_acf_profile_rows, bprx_acf_score_rows_block and the model methods and the CLI flag on top of them.

Inputs (acf_fold_in_ref.case, checked without a GPU by tests/test_acf_fold_in_cpu.py): I = 60 items, C = 8, 40 new users with
history lengths 0, 1, 2, 3, 4, 5, 9, 40 (one history with a repeated item) and 0, 1, 3, 4, 5, 17, 64, 65, 200 pairs; one user with
3 000 consistent pairs, more than any LDS cache holds; a duplicated pair and an i == j pair; a history without pairs; pairs without
a history.  bf16 input sets carry projection weights that a bf16-feature handle holds exactly (acf_fold_in_ref.case); one more
set keeps arbitrary fp32 weights and is held against wider, stated bounds (test_bf16_features_with_arbitrary_projection_weights).

Allowance (the project's rule): allow = 32 x the median over the users with pairs of the float32 restatement's per-user max-abs
deviation from float64, never below one float32 ulp of the largest row magnitude.  Every unexposed user (float64 min |relu input|
>= RELU_DELTA over both levels and all steps) is within it; the exposed ones (at most 10 %, asserted on the CPU) are finite.  Loss:
1e-5 relative for the unexposed users.  Every check prints its triple (float32 deviation / allowance / GPU deviation) and the
left-out count.  What is exact is checked exactly."""
import gc
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import acf_fold_in_ref as R
from fashionvisualexpl_recommend_amd import _ffi

pytestmark = pytest.mark.gpu

TRAINED_LENS = [2, 0, 3, 1, 40, 3]                           # training histories of the handle's own U_TRAINED users


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _trained_lists(seed=5):
    rs = np.random.RandomState(seed)
    lists = [sorted(rs.choice(R.I_ITEMS, n, replace=False).tolist()) if n else [] for n in TRAINED_LENS]
    return lists, [l + [int(rs.randint(R.I_ITEMS))] for l in lists]          # training, evaluation (training + one more)


def _engine(c, **kw):
    from test_gpu_acf import _engine as acf_engine
    train, ev = _trained_lists()
    return acf_engine(c["t"], c["F"], train, "bf16" if c["dtype"] == "bf16raw" else c["dtype"], eval_lists=ev, **kw)


def _hp(shape, which):
    r, kn = R.RUNS[which], R.KNOBS[shape]
    return dict(steps=r["steps"], optimizer=r["optimizer"], lr=kn["lr_adam" if which == "adam" else "lr"], reg=kn["reg"])


def _fold(e, hists, ptr, pos, neg, G0, **hp):
    """One bprx_acf_fold_in call from the start rows G0: (Gu, loss) as numpy arrays."""
    Gu = torch.as_tensor(np.ascontiguousarray(G0), device="cuda")
    loss = e.acf_fold_in(ptr, pos, neg, hp["steps"], Gu, lists=hists, lr=hp["lr"], reg=hp["reg"], optimizer=hp["optimizer"])
    return Gu.cpu().numpy(), loss.cpu().numpy()


def _sub(c, users):
    """The call for the listed users only, in the listed order: (hists, ptr, pos, neg, G0)."""
    users = list(users)
    ptr = c["ptr"]
    cnt = [int(ptr[u + 1] - ptr[u]) for u in users]
    p = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    take = np.concatenate([np.arange(ptr[u], ptr[u + 1]) for u in users] + [np.zeros(0, np.int64)]).astype(np.int64)
    return [c["hists"][u] for u in users], p, c["pos"][take], c["neg"][take], c["G0"][users]


def check_rows(tag, has, r64, r32, got):
    """The allowance rule of the module docstring for the rows `got` [n, k]; returns allow."""
    allow, dev32 = R.allowance(r64, r32, has)
    gdev = np.abs(got.astype(np.float64) - r64["Gu"]).max(1)
    exposed = has & (r64["min_relu"] < R.RELU_DELTA)
    ok = has & ~exposed
    print("%s: float32 deviation %.3e (median; max %.3e) / allowance %.3e / GPU deviation %.3e over the unexposed users, %.3e over "
          "all; left out %d of %d users with pairs" % (tag, np.median(dev32[has]), dev32[has].max(), allow, gdev[ok].max(),
                                                       gdev[has].max(), exposed.sum(), has.sum()))
    assert np.isfinite(got).all(), tag
    assert (gdev[ok] <= allow).all(), (tag, np.nonzero(ok & ~(gdev <= allow))[0], gdev[ok & ~(gdev <= allow)], allow)
    return allow


def check_loss(tag, has, r64, got):
    ok = has & ~(r64["min_relu"] < R.RELU_DELTA)
    err = np.abs(got.astype(np.float64) - r64["loss"])
    print("%s: loss relative error up to %.3e" % (tag, (err[ok] / np.maximum(np.abs(r64["loss"][ok]), 1e-30)).max()))
    assert np.isfinite(got).all() and (err[ok] <= 1e-5 * np.abs(r64["loss"][ok])).all(), (tag, np.nonzero(ok & (err > 1e-5 * np.abs(r64["loss"])))[0])


_cache = {}


def _case(shape, dtype):
    """Inputs, engine and the GPU's results of every run of one input set: made once, never changed."""
    if (shape, dtype) not in _cache:
        c = dict(R.case(shape, dtype))
        c["e"] = _engine(c)
        for which in ("sgd", "adam") if shape in R.NONLINEAR else ("sgd2",):
            c[which] = _fold(c["e"], c["hists"], c["ptr"], c["pos"], c["neg"], c["G0"], **_hp(shape, which))
        c["e"].sync_check()
        _cache[(shape, dtype)] = c
    return _cache[(shape, dtype)]


# ---- against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype,which", R.gpu_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_rows_and_loss_against_float64(shape, dtype, which):
    c = _case(shape, dtype)
    has = np.diff(c["ptr"]) > 0
    tag = "%s %s %s" % (shape, dtype, which)
    got, loss = c[which]
    r64, r32 = R.run(shape, dtype, which), R.run(shape, dtype, which, torch.float32)
    check_rows(tag, has, r64, r32, got)
    check_loss(tag, has, r64, loss)
    assert (~has).sum() == 3 and len(c["hists"][-1]) == 9            # (among them the user with a history and no pairs)
    assert not loss[~has].any() and np.array_equal(_bits(got[~has]), _bits(c["G0"][~has]))      # no pairs: the row stays, loss 0


@pytest.mark.parametrize("shape,dtype,which", R.RAW_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_bf16_features_with_arbitrary_projection_weights(shape, dtype, which):
    """What a user binds: bf16 features and fp32 [Wci | Wix] that are NOT sums of two bf16 halves.  The handle makes Z from the
    two-half weights (k_acf_wcat, 16 mantissa bits), so the rows are held (1) against float64 fed the weights as the handle holds
    them, under the plain allowance, and (2) against float64 on the exact weights under a wider, per-user bound: the allowance plus
    what those 16 bits move the float64 rows by (float64 held - float64 exact; up to 2.5e-06 under Adam, more than the allowance
    itself).  Both bounds come from the restatement alone."""
    c = _case(shape, dtype)
    has = np.diff(c["ptr"]) > 0
    tag = "%s %s %s" % (shape, dtype, which)
    got, loss = c[which]
    r64 = R.run(shape, dtype, which)
    h64, h32 = R.run(shape, dtype, which, held=True), R.run(shape, dtype, which, torch.float32, held=True)
    allow = check_rows(tag + ", weights as held", has, h64, h32, got)
    check_loss(tag + ", weights as held", has, h64, loss)
    moved = np.abs(h64["Gu"] - r64["Gu"]).max(1)
    gdev = np.abs(got.astype(np.float64) - r64["Gu"]).max(1)
    ok = has & ~(r64["min_relu"] < R.RELU_DELTA) & ~(h64["min_relu"] < R.RELU_DELTA)
    print("%s, exact weights: 16 mantissa bits move the float64 rows by up to %.3e (%.2f x the allowance %.3e) / GPU deviation "
          "%.3e" % (tag, moved[has].max(), moved[has].max() / allow, allow, gdev[ok].max()))
    assert (gdev[ok] <= allow + moved[ok]).all(), (tag, np.nonzero(ok & ~(gdev <= allow + moved))[0])
    assert np.array_equal(_bits(got[~has]), _bits(c["G0"][~has]))


def test_users_without_history_are_the_bprmf_problem():
    """Pairs and no history: bprx_fold_in on a plain BPRMF handle with the same Gi and Bi = 0, within the allowance."""
    from fashionvisualexpl_recommend_amd.engine import Engine
    shape = (16, 8, 4, 3)
    c = _case(shape, "fp32")
    has = np.diff(c["ptr"]) > 0
    users = [u for u in range(len(has)) if has[u] and not c["hists"][u]]
    assert len(users) >= 2
    t = c["t"]
    plain = Engine(model="bprmf", num_users=R.U_TRAINED, num_items=R.I_ITEMS, embed_k=shape[0], optimizer="sgd", max_batch=8)
    plain.bind(t["Gu"], t["Gi"], np.zeros(R.I_ITEMS, np.float32))
    for which in ("sgd", "adam"):
        hp = _hp(shape, which)
        _, ptr, pos, neg, G0 = _sub(c, users)
        Gu = torch.as_tensor(np.ascontiguousarray(G0), device="cuda")
        loss = plain.fold_in(ptr, pos, neg, hp["steps"], Gu, None, lr=hp["lr"], reg=hp["reg"], optimizer=hp["optimizer"])
        allow, _ = R.allowance(R.run(shape, "fp32", which), R.run(shape, "fp32", which, torch.float32), has)
        gap = np.abs(Gu.cpu().numpy().astype(np.float64) - c[which][0][users]).max()
        print("no history, %s: bprx_fold_in - bprx_acf_fold_in %.3e / allowance %.3e" % (which, gap, allow))
        assert gap <= allow
        assert np.allclose(loss.cpu().numpy(), c[which][1][users], rtol=1e-5, atol=0)
    plain.sync_check()
    plain.close()


# ---- bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", [((16, 8, 4, 6), "bf16"), ((130, 32, 64, 49), "fp32")], ids=lambda v: str(v).replace(" ", ""))
def test_a_users_bits_depend_on_nothing_but_the_user(monkeypatch, shape, dtype):
    c = _case(shape, dtype)
    e, n = c["e"], len(c["hists"])
    runs = ("sgd", "adam") if shape in R.NONLINEAR else ("sgd2",)
    for which in runs:
        hp = _hp(shape, which)
        rows, loss = c[which]
        again = _fold(e, c["hists"], c["ptr"], c["pos"], c["neg"], c["G0"], **hp)
        assert np.array_equal(_bits(rows), _bits(again[0])) and np.array_equal(_bits(loss), _bits(again[1])), "two calls"
        perm = np.random.RandomState(7).permutation(n)
        shuffled = _fold(e, *_sub(c, perm), **hp)
        assert np.array_equal(_bits(shuffled[0]), _bits(rows[perm])) and np.array_equal(_bits(shuffled[1]), _bits(loss[perm]))
        for users in ([0], [35], [37], [n - 1], range(4), range(20, 25)):       # n = 1, 4, 5
            users = list(users)
            part = _fold(e, *_sub(c, users), **hp)
            assert np.array_equal(_bits(part[0]), _bits(rows[users])), (which, users)
            assert np.array_equal(_bits(part[1]), _bits(loss[users])), (which, users)
    monkeypatch.setenv("BPRX_FOLD_CACHE", "0")                                   # read at create: every pair is gathered every step
    e0 = _engine(c)
    for which in runs:
        plain = _fold(e0, c["hists"], c["ptr"], c["pos"], c["neg"], c["G0"], **_hp(shape, which))
        assert np.array_equal(_bits(plain[0]), _bits(c[which][0])) and np.array_equal(_bits(plain[1]), _bits(c[which][1])), which
    e0.sync_check()
    e0.close()


@pytest.mark.parametrize("shape,dtype", [((16, 8, 4, 3), "fp32"), ((20, 96, 32, 130), "fp32"), ((5, 3, 2, 1), "bf16")],
                         ids=lambda v: str(v).replace(" ", ""))
def test_row_calls_on_the_handles_own_rows_are_the_user_calls(shape, dtype):
    """bprx_acf_profile_rows / bprx_acf_score_rows_block with slices of the handle's own Gu and of its CSRs: the bits of
    bprx_acf_profiles / bprx_score_block, also for a row range inside a larger table."""
    c = _case(shape, dtype)
    e, U = c["e"], R.U_TRAINED
    train, ev = _trained_lists()
    want_p = e.acf_profiles(range(U))
    assert torch.equal(want_p.view(torch.int32), e.acf_profile_rows(e.t["Gu"], csr=e.acf_train).view(torch.int32))
    for u0, u1 in ((0, U), (3, 4), (2, 5)):
        got = e.acf_profile_rows(e.t["Gu"][u0:u1].contiguous(), lists=train[u0:u1])
        assert torch.equal(want_p[u0:u1].view(torch.int32), got.view(torch.int32)), (u0, u1)
        want_x = e.score_block(u0, u1)
        got_x = e.acf_score_rows_block(e.t["Gu"][u0:u1].contiguous(), 0, u1 - u0, lists=ev[u0:u1])
        assert torch.equal(want_x.view(torch.int32), got_x.view(torch.int32)), (u0, u1)
        in_x = e.acf_score_rows_block(e.t["Gu"], u0, u1, csr=e.acf_eval)         # a row range of a larger table
        assert torch.equal(want_x.view(torch.int32), in_x.view(torch.int32)), (u0, u1)
    e.sync_check()


# ---- behaviour -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 8, 4, 3), (64, 64, 64, 70)], ids=lambda v: str(v).replace(" ", ""))
def test_one_sgd_step_moves_a_trained_users_row_as_the_full_step_does(shape):
    """steps = 1, sgd, from a trained user's row with that user's training history, against bprx_step in BPRX_ACF_GRAD_FULL on the
    batch made of that user's pairs on a second handle with identical tables.  The folding handle stays detached."""
    c = R.case(shape, "fp32")
    train, _ = _trained_lists()
    rs = np.random.RandomState(41)
    u, B, lr, reg = 5, 37, 0.05, 1e-3
    pos, neg = rs.randint(R.I_ITEMS, size=B).astype(np.int32), rs.randint(R.I_ITEMS, size=B).astype(np.int32)
    pos[3], neg[3] = pos[2], neg[2]
    neg[7] = pos[7]
    ea, eb = (_engine(c, lr=lr, reg=reg) for _ in range(2))
    eb.acf_set_gradient("full")
    hp = dict(steps=1, lr=lr, reg=reg, optimizer="sgd")
    G0 = c["t"]["Gu"][u:u + 1]
    fold = _fold(ea, [train[u]], [0, B], pos, neg, G0, **hp)[0][0]
    assert ea.acf_gradient() == "detached"
    r64, r32 = (R.fold_in(c["t"], c["F"], [train[u]], [0, B], pos, neg, G0, 1, lr, reg, "sgd", dt)["Gu"][0]
                for dt in (torch.float64, torch.float32))
    dev = lambda x: torch.as_tensor(x, device="cuda")
    eb.step(dev(np.full(B, u, np.int32)), dev(pos), dev(neg))
    stepped = eb.t["Gu"][u].cpu().numpy()
    d32 = float(np.abs(r32 - r64).max())
    allow = max(R.TOL_MULT * d32, float(np.spacing(np.float32(np.abs(r64).max()))))
    gap = float(np.abs(stepped.astype(np.float64) - fold).max())
    print("T=1 %s: float32 deviation %.3e / allowance %.3e / fold_in - float64 %.3e / bprx_step - float64 %.3e / bprx_step - "
          "fold_in %.3e" % (shape, d32, allow, np.abs(fold - r64).max(), np.abs(stepped - r64).max(), gap))
    assert np.abs(stepped - G0[0]).max() > 1e-3                                   # (the step moved the row)
    assert gap <= allow and np.abs(fold - r64).max() <= allow
    assert ea.acf_gradient() == "detached" and eb.acf_gradient() == "full"
    for e in (ea, eb):
        e.sync_check()
        e.close()


def test_a_step_between_two_folds_is_seen_by_the_second():
    """Fold, one bprx_step, fold again: the second fold runs on the moved tables (Z / GP are prepared again by every call)."""
    shape = (16, 8, 4, 3)
    c = R.case(shape, "fp32")
    e = _engine(c, lr=0.2, reg=1e-3)
    hp = _hp(shape, "sgd")
    users = [7, 12, 20, 27, 33, 36, 39, 1]
    sub = _sub(c, users)
    first = _fold(e, *sub, **hp)[0]
    rs = np.random.RandomState(78)
    dev = lambda x: torch.as_tensor(x, device="cuda")
    e.step(dev(rs.randint(0, R.U_TRAINED, 64).astype(np.int32)), dev(rs.randint(0, R.I_ITEMS, 64).astype(np.int32)),
           dev(rs.randint(0, R.I_ITEMS, 64).astype(np.int32)))
    second, loss = _fold(e, *sub, **hp)
    assert not np.array_equal(_bits(first), _bits(second))                        # (the step moved what the fold reads)
    t2 = {n: e.t[n].cpu().numpy() for n in R.FROZEN}
    r64, r32 = (R.fold_in(t2, c["F"], *sub, hp["steps"], hp["lr"], hp["reg"], hp["optimizer"], dt) for dt in (torch.float64, torch.float32))
    has = np.diff(sub[1]) > 0
    check_rows("fold / step / fold", has, r64, r32, second)
    check_loss("fold / step / fold", has, r64, loss)
    e.sync_check()
    e.close()


def test_errors_leave_the_handle_usable_and_no_allocation_behind():
    from fashionvisualexpl_recommend_amd.engine import Engine
    from attentive_ref import random_inputs, random_tables as af_tables
    from test_gpu_attentive import _engine as af_engine
    lib = _ffi.lib()
    gc.collect()
    live = lib.bprx_live_device_allocs()
    shape = (16, 8, 4, 3)
    k, I = shape[0], R.I_ITEMS
    c = R.case(shape, "fp32")
    t = c["t"]
    e = _engine(c)
    rs = np.random.RandomState(71)
    plain = Engine(model="bprmf", num_users=R.U_TRAINED, num_items=I, embed_k=k, optimizer="sgd", max_batch=8).bind(t["Gu"], t["Gi"], t["Bi"])
    Fv = np.abs(rs.standard_normal((I, 32))).astype(np.float32)
    vbpr = Engine(model="vbpr", num_users=R.U_TRAINED, num_items=I, embed_k=k, embed_d=4, feat_dim=32, feat_dtype="fp32", optimizer="sgd",
                  max_batch=8).bind(Gu=t["Gu"], Gi=t["Gi"], Bi=t["Bi"], Tu=np.zeros((R.U_TRAINED, 4), np.float32), F=Fv / Fv.max(),
                                    E=np.zeros((32, 4), np.float32), Bp=np.zeros(32, np.float32))
    unbound = Engine(model="bprmf", num_users=R.U_TRAINED, num_items=I, embed_k=k, optimizer="sgd", max_batch=8)
    af = af_engine(af_tables(rs, 4, 6, k, 9, 5, 12), random_inputs(rs, 6, 9, 5), optimizer="sgd", lr=0.05, reg=1e-3, B=8, rate=0.0)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    hp_, hi = dev(np.array([0, 2, 3], np.int64)), dev(np.array([5, 9, 7], np.int32))
    ptr, pos, neg = dev(np.array([0, 2, 3], np.int64)), dev(np.array([1, 2, 3], np.int32)), dev(np.array([4, 5, 6], np.int32))
    Gu, loss = torch.zeros((2, k), device="cuda"), torch.zeros(2, device="cuda")
    sc, pr = torch.zeros((2, I), device="cuda"), torch.zeros((2, k), device="cuda")
    p = lambda x: None if x is None else x.data_ptr()

    def call(hd, n=2, steps=1, opt=0, hp=hp_, hi_=hi, ptr_=ptr, pos_=pos, neg_=neg, Gu_=Gu, loss_=loss):
        return lib.bprx_acf_fold_in(hd, p(hp), p(hi_), p(ptr_), p(pos_), p(neg_), n, steps, 0.05, 1e-3, opt, p(Gu_), p(loss_), None)

    assert call(e.h) == 0
    torch.cuda.synchronize()
    held = lib.bprx_live_device_allocs()
    good = Gu.cpu().numpy().copy()
    assert np.abs(good).max() > 0
    Gu.zero_()
    assert call(e.h, loss_=None) == 0 and np.array_equal(_bits(good), _bits(Gu.cpu().numpy()))      # loss is optional
    assert call(e.h, n=0) == 0 and call(e.h, n=0, hi_=None, pos_=None, neg_=None) == 0
    for kw in (dict(n=-1), dict(steps=0), dict(opt=2), dict(hp=None), dict(hi_=None), dict(ptr_=None), dict(pos_=None), dict(neg_=None),
               dict(Gu_=None)):
        assert call(e.h, **kw) == _ffi.E_INVALID, kw
    for other in (plain, vbpr, af):
        assert call(other.h) == _ffi.E_INVALID and "bprx_bind_acf" in lib.bprx_last_error(other.h).decode()
    assert call(unbound.h) == _ffi.E_STATE
    rows = lambda hd, G=Gu, n=2, r0=0, r1=2, out=sc, hp=hp_, hi_=hi: lib.bprx_acf_score_rows_block(hd, p(G), n, p(hp), p(hi_), r0, r1, p(out), None)
    prof = lambda hd, G=Gu, n=2, out=pr, hp=hp_, hi_=hi: lib.bprx_acf_profile_rows(hd, p(G), n, p(hp), p(hi_), p(out), None)
    assert rows(e.h) == 0 and rows(e.h, r0=1, r1=1, G=None, out=None, hp=None, hi_=None) == 0
    assert prof(e.h) == 0 and prof(e.h, n=0, G=None, out=None, hi_=None) == 0
    for kw in (dict(n=-1), dict(r0=-1), dict(r1=3), dict(r0=2, r1=1), dict(G=None), dict(out=None), dict(hp=None), dict(hi_=None)):
        assert rows(e.h, **kw) == _ffi.E_INVALID, kw
    for kw in (dict(n=-1), dict(G=None), dict(out=None), dict(hp=None), dict(hi_=None)):
        assert prof(e.h, **kw) == _ffi.E_INVALID, kw
    for other in (plain, vbpr, af):
        assert rows(other.h) == _ffi.E_INVALID and prof(other.h) == _ffi.E_INVALID
    assert rows(unbound.h) == _ffi.E_STATE and prof(unbound.h) == _ffi.E_STATE
    # the pinned rejections of the other fold-in entries on the ACF handle stay
    assert lib.bprx_fold_in(e.h, p(ptr), p(pos), p(neg), 2, 1, 0.05, 1e-3, 0, p(Gu), None, p(loss), None) == _ffi.E_INVALID
    assert lib.bprx_score_rows_block(e.h, p(Gu), None, 2, 0, 2, p(sc), None) == _ffi.E_INVALID
    assert lib.bprx_af_fold_in(e.h, p(ptr), p(pos), p(neg), 2, 1, 0.05, 1e-3, 0, p(Gu), p(loss), None) == _ffi.E_INVALID
    assert lib.bprx_af_score_rows_block(e.h, p(Gu), 2, 0, 2, p(sc), None, None) == _ffi.E_INVALID
    e.sync_check()
    # item ids out of range, in the history and in the pairs: clamped, and reported by sync_check (once); the handle goes on working
    for kw_bad, kw_clamped in ((dict(hi_=dev(np.array([5, I + 3, 7], np.int32))), dict(hi_=dev(np.array([5, I - 1, 7], np.int32)))),
                               (dict(pos_=dev(np.array([1, I, 3], np.int32))), dict(pos_=dev(np.array([1, I - 1, 3], np.int32)))),
                               (dict(neg_=dev(np.array([4, -7, 6], np.int32))), dict(neg_=dev(np.array([4, 0, 6], np.int32))))):
        Gu.zero_()
        assert call(e.h, **kw_bad) == 0
        with pytest.raises(_ffi.BprxError) as err:
            e.sync_check()
        assert err.value.code == _ffi.E_RANGE
        e.sync_check()                                                   # reported once
        clamped = Gu.cpu().numpy().copy()
        Gu.zero_()
        assert call(e.h, **kw_clamped) == 0
        assert np.array_equal(_bits(clamped), _bits(Gu.cpu().numpy()))
        e.sync_check()
    Gu.zero_()
    assert call(e.h) == 0 and np.array_equal(_bits(good), _bits(Gu.cpu().numpy()))
    e.sync_check()
    assert lib.bprx_live_device_allocs() == held                     # the calls allocated nothing
    # a block of more rows than max_batch: one profile workspace, allocated once and reused
    nbig = e.max_batch + 44
    big = e.t["Gu"][torch.arange(nbig, device="cuda") % R.U_TRAINED].contiguous()
    _, ev = _trained_lists()
    csr = e.csr([ev[r % R.U_TRAINED] for r in range(nbig)])
    x = e.acf_score_rows_block(big, 0, nbig, csr=csr)
    assert lib.bprx_live_device_allocs() == held + 1
    want = e.score_block(0, R.U_TRAINED)
    assert torch.equal(x.view(torch.int32), want[torch.arange(nbig, device="cuda") % R.U_TRAINED].view(torch.int32))
    e.acf_score_rows_block(big, 0, nbig, csr=csr)
    e.acf_score_rows_block(big, 3, nbig - 2, csr=csr)
    assert lib.bprx_live_device_allocs() == held + 1
    # a shape whose walk does not fit a workgroup's LDS: rejected by the fold, the forward calls still run
    from acf_ref import random_tables as acf_tables
    from test_gpu_acf import _engine as acf_engine
    wide = acf_engine(acf_tables(rs, 2, 4, 512, 8, 16, 16), np.abs(rs.standard_normal((4, 2048, 8))).astype(np.float32), [[0, 1], [2]])
    Gw = torch.zeros((2, 512), device="cuda")
    assert lib.bprx_acf_fold_in(wide.h, p(hp_), p(hi % 4), p(ptr), p(pos % 4), p(neg % 4), 2, 1, 0.05, 1e-3, 0, p(Gw), None, None) == _ffi.E_INVALID
    assert "LDS" in lib.bprx_last_error(wide.h).decode()
    wide.sync_check()
    for eng in (e, plain, vbpr, unbound, af, wide):
        eng.close()
    assert lib.bprx_live_device_allocs() == live


# ---- the model and the files ---------------------------------------------------------------------------------------------------------
def _toy_model(rs, U=40, I=50, K=5):
    from fashionvisualexpl_recommend_amd import models, synth
    train, val, test = synth.make_interactions(U, I, per_user=8, seed=7)
    data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=val, test_list=test,
                     params=Namespace(batch_eval=128))
    params = Namespace(epochs=1, batch_size=32, embed_k=16, lr=0.05, reg=1e-3, top_k=K, dataset="toy", rec="acf",
                       layers_component=[32, 1], layers_item=[32, 1], optimizer="sgd", dtype="fp32")
    return models.ACF(data, params, features=np.abs(rs.standard_normal((I, 4, 64))).astype(np.float32)), train


def test_recommend_new_users_masks_histories_and_matches_numpy():
    K = 5
    m, train = _toy_model(np.random.RandomState(23), K=K)
    hist = [list(h) for h in train[:12]] + [[]]                      # a user without history: the zero row, every score equal
    fold = dict(steps=6, negatives=3, seed=3)
    idx, val_ = m.recommend_new_users(hist, **fold)
    assert idx.shape == val_.shape == (13, K)
    Gu = m.fold_in_users(hist, **fold)
    assert tuple(Gu.shape) == (13, 16) and not Gu[12].any() and Gu[:12].abs().amax(1).min().item() > 0    # a zero start is live
    sc = m.engine.acf_score_rows_block(Gu, 0, 13, lists=hist).cpu().numpy()
    for r in range(13):
        row = sc[r].copy()
        row[hist[r]] = -np.inf
        if r == 12:                                                  # the tie row: numpy's own order on the GPU's row
            assert len(set(row.tolist())) == 1
            want = row.argsort()[-K:][::-1]
        else:
            want = np.argsort(-row, kind="stable")[:K]
            gaps = row[want][:-1] - row[want][1:]
            assert (gaps > 0).all() and row[want[-1]] > np.sort(row)[-K - 1]       # (no tie decides this list)
        assert np.array_equal(idx[r], want), r
        assert np.array_equal(_bits(val_[r]), _bits(sc[r][want])), r
        assert not set(idx[r].tolist()) & set(hist[r])
    # steps = 0: the start rows, no kernel call; scored with the history they give the history-only profile
    init = np.random.RandomState(3).standard_normal((13, 16)).astype(np.float32)
    assert not m.fold_in_users(hist, steps=0).any()
    assert np.array_equal(_bits(m.fold_in_users(hist, steps=0, init=init).cpu().numpy()), _bits(init))
    with pytest.raises(_ffi.BprxError):
        m.engine.acf_fold_in([0] * 14, [], [], 0, torch.zeros((13, 16), device="cuda"), lists=hist)      # the library itself wants steps >= 1
    m.engine.sync_check()
    m.engine.close()


def test_cli_writes_new_user_files(tmp_path):
    from fashionvisualexpl_recommend_amd import train_rec
    from test_gpu_acf import _write_dataset
    root, train, val, maps = _write_dataset(tmp_path)
    res, top_k = str(tmp_path / "res"), 5
    hist = {"new shopper": [3, 9, 20], "b": [7], "c 3": [5, 6, 5]}
    rows = [("new shopper", 3), ("b", 7), ("new shopper", 9), ("c 3", 5), ("c 3", 6), ("new shopper", 20), ("c 3", 5)]
    (tmp_path / "new.tsv").write_text("".join("%s\t%d\n" % r for r in rows))
    train_rec.train(["--rec", "acf", "--dataset", "toy", "--data_root", root, "--results_root", res, "--epochs", "2",
                     "--batch_size", "64", "--embed_k", "16", "--layers_component", "32", "1", "--layers_item", "16", "1",
                     "--reg", "0.01", "--top_k", str(top_k), "--acf_new_users", str(tmp_path / "new.tsv"), "--fold_steps", "9",
                     "--fold_negatives", "3"])
    rdir = os.path.join(res, "rec_results", "toy", "acf")
    files = sorted(os.listdir(rdir))
    base = [f for f in files if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(base) == 2
    for f in base:
        new = f.replace("recs-", "new-user-recs-", 1)
        assert new in files
        got = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir, new))]
        assert len(got) == 3 * top_k and all(len(r) == 3 for r in got)       # label  i  score
        assert [r[0] for r in got] == [lab for lab in ("new shopper", "b", "c 3") for _ in range(top_k)]     # one block per label, file order
        for q, lab in enumerate(("new shopper", "b", "c 3")):
            blk = got[q * top_k:(q + 1) * top_k]
            s = [float(r[2]) for r in blk]
            assert s == sorted(s, reverse=True) and len({r[1] for r in blk}) == top_k
            assert all(0 <= int(r[1]) < 80 for r in blk) and not {int(r[1]) for r in blk} & set(hist[lab])
