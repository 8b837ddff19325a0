"""Warm items on the MI355X against the float64 restatement (tests/item_fold_ref.py): bprx_fold_in_items, bprx_score_warm_block,
bprx_audience_warm_block, the model methods on top of them and the files of train_rec --warm_items.

Allowance per compared output (the project's rule, tests/test_gpu_new_items.py): 32 x the max-abs deviation of the FLOAT32
restatement from the float64 one over the case, never below one float32 ulp of the output's largest magnitude.  Every check prints
its triple (float32 deviation / allowance / GPU deviation).  What is exact is checked exactly: two calls, an item's rows wherever it
stands and whatever n is, the cached against the re-gathering form, the warm score blocks against their catalogue twins.

Inputs (tests/item_fold_cases.py, checked on the CPU by tests/test_item_fold_cpu.py with host-made projections): U = I = 300, tables
~ N(0, 0.3), 130 new items with 0, 1, 3, 4, 5, 17, 64, 65, 200 and 1..40 random pairs, roles mixed, a duplicated pair and one (u, o)
in both roles among them, and one item with 3 000 pairs, past any LDS share.  sgd: 20 steps at lr = 0.002 (the batch loss is summed:
at lr = 0.02 items with 200 and 3 000 pairs oscillate in float64); Adam: 3 steps at lr = 0.05.  On the CPU, three seeds per width:
the float64 loss falls for every item, float32 rows deviate by 2e-7 .. 5e-7 under sgd, Adam's left-out share is 0.5 .. 1.4 %."""
import gc
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import item_fold_cases as C
import item_fold_ref as R
from fashionvisualexpl_recommend_amd import _ffi, synth
from test_gpu_feat_explain import _bits, _snapshot, _tables, _unique_batches, _vbpr

pytestmark = pytest.mark.gpu

U, I, BIG = C.U, C.I, C.BIG
SGD, ADAM = C.SGD, C.ADAM


def _allow(r64, r32):
    dev = float(np.abs(r64 - r32.astype(np.float64)).max())
    return dev, max(32.0 * dev, float(np.spacing(np.float32(np.abs(r64).max()))))


def _report(tag, r64, r32, got):
    dev, allow = _allow(r64, r32)
    gdev = float(np.abs(got.astype(np.float64) - r64).max())
    print("%s: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (tag, dev, allow, gdev))
    return gdev, allow


def _engine(t, optimizer="sgd", B=64, dtype="fp32", **kw):
    from fashionvisualexpl_recommend_amd.engine import Engine
    nu, k = t["Gu"].shape
    if "F" not in t:
        return Engine(model="bprmf", num_users=nu, num_items=t["Gi"].shape[0], embed_k=k, optimizer=optimizer, lr=0.05, reg=1e-3,
                      max_batch=B, **kw).bind(t["Gu"], t["Gi"], t["Bi"])
    D, d = t["E"].shape
    return Engine(model="vbpr", num_users=nu, num_items=t["Gi"].shape[0], embed_k=k, embed_d=d, feat_dim=D, feat_dtype=dtype,
                  optimizer=optimizer, lr=0.05, reg=1e-3, max_batch=B, **kw).bind(**C.bound(t))


def _proj(e, F):
    """(device [n, PS], numpy [n, d + 1]) projections of a feature table, (None, None) without a visual part."""
    if not e.d:
        return None, None
    P = e.project_rows(F)
    return P, P.cpu().numpy()[:, :e.d + 1]


def _fold(e, Pn, ptr, user, other, role, W0, **hp):
    """One bprx_fold_in_items call from the start rows W0 [n, k + 1]: (Gi, Bi, loss) as numpy arrays."""
    k = e.k
    Gi = torch.as_tensor(np.ascontiguousarray(W0[:, :k]), device="cuda")
    Bi = torch.as_tensor(np.ascontiguousarray(W0[:, k]), device="cuda")
    loss = e.fold_in_items(ptr, user, other, role, hp["steps"], Gi, Bi, Pn, lr=hp["lr"], reg=hp["reg"], optimizer=hp["optimizer"])
    return Gi.cpu().numpy(), Bi.cpu().numpy(), loss.cpu().numpy()


def _sub(Pn, ptr, user, other, role, W0, which):
    """The call for the listed items only, in the listed order."""
    which = list(which)
    cnt = [int(ptr[r + 1] - ptr[r]) for r in which]
    p = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in which] + [np.zeros(0, np.int64)]).astype(np.int64)
    return (None if Pn is None else Pn[which].contiguous()), p, user[take], other[take], role[take], W0[which]


_cache = {}


def _case(k, d):
    """Tables, engine, items, both restatements (sgd, adam) and the GPU's n = 130 results of one width: made once, never changed."""
    if (k, d) not in _cache:
        seed = C.SEEDS[(k, d)]
        t = C.tables(k, d, seed)
        e = _engine(t)
        _, P = _proj(e, t.get("F"))
        Pn_dev, Pn = _proj(e, t.get("Fn"))
        a = C.items(t, P, Pn, k, d, seed)
        c = dict(t=t, e=e, P=P, Pn=Pn, Pn_dev=Pn_dev, a=a, ptr=a[0])
        for name, hp in (("sgd", SGD), ("adam", ADAM)):
            c[name + "64"], c[name + "32"] = (C.restate(t, P, Pn, *a, hp, dt) for dt in (np.float64, np.float32))
            c[name + "_gpu"] = _fold(e, Pn_dev, *a, **hp)
        e.sync_check()
        _cache[(k, d)] = c
    return _cache[(k, d)]


# ---- against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", C.WIDTHS)
def test_sgd_rows_and_loss_against_float64(k, d):
    c = _case(k, d)
    r64, r32, got = c["sgd64"], c["sgd32"], c["sgd_gpu"]
    gdev, allow = _report("sgd rows k=%d d=%d" % (k, d), C.rows(r64), C.rows(r32), C.rows(got))
    assert gdev <= allow
    ldev, lallow = _report("sgd loss_20 k=%d d=%d" % (k, d), r64["loss"], r32["loss"], got[2])
    assert ldev <= lallow
    first = _fold(c["e"], c["Pn_dev"], *c["a"], **dict(SGD, steps=1))[2]
    fdev, fallow = _report("sgd loss_1 k=%d d=%d" % (k, d), r64["loss_first"], r32["loss_first"], first)
    assert fdev <= fallow
    has = np.diff(c["ptr"]) > 0
    assert (r64["loss"][has] < r64["loss_first"][has]).all()                      # the definition itself, on these inputs
    assert (got[2][has] < first[has]).all(), np.nonzero(~(got[2] < first) & has)[0]
    assert got[2][0] == 0 and np.array_equal(_bits(C.rows(got)[0]), _bits(c["a"][4][0]))    # no pairs: the rows stay, loss 0


@pytest.mark.parametrize("k,d", C.WIDTHS)
def test_adam_rows_against_float64(k, d):
    """Entries (item, element) whose float64 |g| at any step is below 1e-3 of that item's largest |g| at that step are left out
    (item_fold_cases.adam_keep); at most 2 % of them may be."""
    c = _case(k, d)
    r64, r32, got = c["adam64"], c["adam32"], c["adam_gpu"]
    keep, share = C.adam_keep(r64, c["ptr"])
    print("adam k=%d d=%d: left-out share %.4f" % (k, d, share))
    assert share <= 0.02
    gdev, allow = _report("adam rows k=%d d=%d" % (k, d), C.rows(r64)[keep], C.rows(r32)[keep], C.rows(got)[keep])
    assert gdev <= allow
    ldev, lallow = _report("adam loss_3 k=%d d=%d" % (k, d), r64["loss"], r32["loss"], got[2])
    assert ldev <= lallow
    first = _fold(c["e"], c["Pn_dev"], *c["a"], **dict(ADAM, steps=1))[2]
    fdev, fallow = _report("adam loss_1 k=%d d=%d" % (k, d), r64["loss_first"], r32["loss_first"], first)
    assert fdev <= fallow
    has = np.diff(c["ptr"]) > 0
    assert (got[2][has] < first[has]).all(), np.nonzero(~(got[2] < first) & has)[0]
    assert got[2][0] == 0 and np.array_equal(_bits(C.rows(got)[0]), _bits(c["a"][4][0]))


@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
@pytest.mark.parametrize("k,d", [(5, 0), (16, 12), (64, 64)])
def test_one_step_moves_a_catalogue_items_rows_as_bprx_step_does(k, d, opt):
    """T = 1 from a catalogue item's own Gi / Bi / P row against the engine's own step on a batch that has the item once per
    triplet, in either role (adam_tf23 at adam_step = 0)."""
    t = C.tables(k, d, seed=40 + k)
    e = _engine(t, optimizer=opt)
    P_dev, P = _proj(e, t.get("F"))
    rs = np.random.RandomState(41)
    it, B, lr, reg = 123, 37, 0.05, 1e-3
    user, role = rs.randint(U, size=B).astype(np.int32), rs.randint(2, size=B).astype(np.int32)
    other = rs.choice(np.delete(np.arange(I), it), size=B).astype(np.int32)
    assert 0 < role.sum() < B
    W0 = np.concatenate([t["Gi"][it:it + 1], t["Bi"][it:it + 1, None]], 1)
    hp = dict(steps=1, lr=lr, reg=reg, optimizer=opt)
    Pn_dev = None if P_dev is None else P_dev[it:it + 1].contiguous()
    fold = C.rows(_fold(e, Pn_dev, [0, B], user, other, role, W0, **hp))[0]
    r64, r32 = (C.rows(C.restate(t, P, None if P is None else P[it:it + 1], [0, B], user, other, role, W0, hp, dt))[0]
                for dt in (np.float64, np.float32))
    assert e.adam_step == 0
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device="cuda")
    e.step(dev(user), dev(np.where(role == 0, it, other)), dev(np.where(role == 0, other, it)))
    stepped = np.concatenate([e.t["Gi"][it].cpu().numpy(), e.t["Bi"][it:it + 1].cpu().numpy()])
    _, allow = _allow(r64, r32)
    gap = float(np.abs(stepped.astype(np.float64) - fold).max())
    print("T=1 %s k=%d d=%d: allowance %.3e / fold_in_items - float64 %.3e / bprx_step - float64 %.3e / bprx_step - fold_in_items %.3e" % (
        opt, k, d, allow, np.abs(fold - r64).max(), np.abs(stepped - r64).max(), gap))
    assert np.abs(stepped - W0[0]).max() > 1e-3                                   # (the step moved the rows)
    assert gap <= allow
    e.sync_check()
    e.close()


@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
def test_a_factored_handle_regularises_a_negatives_bias_in_full(opt):
    """GradFashion: c_neg = 1.  T = 1 from a catalogue item's own rows against the factored engine's own step and
    against the restatement with c_neg = 1; reg = 0.1 and |Bi| up to 1 keep the c_neg = 0.1 restatement far outside the allowance."""
    from test_gpu_gradfashion import _engine as _gf_engine, _setup as _gf_setup
    t, F = _gf_setup("fp32")
    e = _gf_engine(t, F, "fp32", optimizer=opt, reg=0.1, B=64)
    P_dev = e.project_rows(F)
    P = P_dev.cpu().numpy()[:, :e.d + 1]
    rs = np.random.RandomState(43)
    it, B, lr, reg, k = 123, 37, 0.05, 0.1, e.k
    user, role = rs.randint(300, size=B).astype(np.int32), rs.randint(2, size=B).astype(np.int32)
    other = rs.choice(np.delete(np.arange(600), it), size=B).astype(np.int32)
    W0 = np.concatenate([t["Gi"][it:it + 1], t["Bi"][it:it + 1, None]], 1)
    fold = C.rows(_fold(e, P_dev[it:it + 1].contiguous(), [0, B], user, other, role, W0, steps=1, lr=lr, reg=reg, optimizer=opt))[0]
    re = lambda c_neg, dt: C.rows(R.fold_in_items(t["Gu"], t["Tu"], t["Gi"], t["Bi"], P, P[it:it + 1], [0, B], user, other, role,
                                                  W0[:, :k], W0[:, k], 1, lr, reg, opt, dt, c_neg=c_neg))[0]
    r64, r32, tenth = re(1.0, np.float64), re(1.0, np.float32), re(0.1, np.float64)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device="cuda")
    e.step(dev(user), dev(np.where(role == 0, it, other)), dev(np.where(role == 0, other, it)))
    stepped = np.concatenate([e.t["Gi"][it].cpu().numpy(), e.t["Bi"][it:it + 1].cpu().numpy()])
    _, allow = _allow(r64, r32)
    print("factored T=1 %s: allowance %.3e / fold_in_items - float64 %.3e / bprx_step - fold_in_items %.3e / c_neg 0.1 - float64 %.3e" % (
        opt, allow, np.abs(fold - r64).max(), np.abs(stepped - fold).max(), np.abs(tenth - r64).max()))
    if opt == "sgd":                                                              # (Adam's first step is a sign step: the factor does not show)
        assert np.abs(tenth - r64).max() > 100 * allow                            # the check tells the two factors apart
    assert np.abs(fold - r64).max() <= allow
    assert float(np.abs(stepped.astype(np.float64) - fold).max()) <= allow
    e.sync_check()
    e.close()


# ---- bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", C.WIDTHS)
def test_an_items_bits_depend_on_nothing_but_the_item(monkeypatch, k, d):
    c = _case(k, d)
    e, Pn, a = c["e"], c["Pn_dev"], c["a"]
    for name, hp in (("sgd", SGD), ("adam", ADAM)):
        full = c[name + "_gpu"]
        rows, loss = C.rows(full), full[2]
        again = _fold(e, Pn, *a, **hp)
        assert np.array_equal(_bits(rows), _bits(C.rows(again))) and np.array_equal(_bits(loss), _bits(again[2])), "two calls"
        perm = np.random.RandomState(7).permutation(C.N_NEW)
        shuffled = _fold(e, *_sub(Pn, *a, perm), **hp)
        assert np.array_equal(_bits(C.rows(shuffled)), _bits(rows[perm])) and np.array_equal(_bits(shuffled[2]), _bits(loss[perm]))
        for which in ([0], [1], [5], [BIG], [8], [129], range(4), range(5)):      # n = 1, 4, 5
            which = list(which)
            part = _fold(e, *_sub(Pn, *a, which), **hp)
            assert np.array_equal(_bits(C.rows(part)), _bits(rows[which])), (name, which)
            assert np.array_equal(_bits(part[2]), _bits(loss[which])), (name, which)
    monkeypatch.setenv("BPRX_FOLD_CACHE", "0")                                    # read at create: every item forms its pairs per step
    e0 = _engine(c["t"])
    Pn0, _ = _proj(e0, c["t"].get("Fn"))
    for name, hp in (("sgd", SGD), ("adam", ADAM)):
        plain = _fold(e0, Pn0, *a, **hp)
        assert np.array_equal(_bits(C.rows(plain)), _bits(C.rows(c[name + "_gpu"]))), name
        assert np.array_equal(_bits(plain[2]), _bits(c[name + "_gpu"][2])), name
    e0.sync_check()
    e0.close()


# ---- the score entries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", [(16, 12), (64, 64), (16, 0), (15, 12), (16, 11), (5, 0)])
def test_warm_blocks_are_the_catalogue_blocks_for_the_catalogues_own_rows(k, d):
    """A slice of the catalogue's own Gi / Bi / P: those columns of score_block and those rows of audience_block, bit for bit for
    even k and d (an odd width: score_warm_block runs score_block's own kernel for it, still the same bits; audience_warm_block
    stays on the matrix unit, like audience_block, whose bits it has -- both are within the allowance of score_block).  Zero
    Gi / Bi rows: the bits of score_new_block."""
    t = C.tables(k, d, seed=80 + k)
    e = _engine(t)
    P_dev, P = _proj(e, t.get("F"))
    S = e.score_block(0, U).cpu().numpy()
    A = e.audience_block(0, I).cpu().numpy()
    r64, r32 = (R.scores(t["Gu"], t.get("Tu"), t["Gi"], t["Bi"], P, dt) for dt in (np.float64, np.float32))
    even = k % 2 == 0 and d % 2 == 0
    for j0, j1 in ((0, I), (7, 8), (120, 259)):
        Gi, Bi = e.t["Gi"][j0:j1].contiguous(), e.t["Bi"][j0:j1].contiguous()
        Pn = P_dev[j0:j1].contiguous() if d else None
        for u0, u1 in ((0, U), (130, 131), (5, 270)):
            got = e.score_warm_block(u0, u1, Gi, Bi, Pn).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(S[u0:u1, j0:j1])), (j0, j1, u0, u1)
        aud = e.audience_warm_block(Gi, Bi, Pn, 0, j1 - j0).cpu().numpy()
        assert np.array_equal(_bits(aud), _bits(A[j0:j1])), (j0, j1)
        if j1 - j0 > 3:
            part = e.audience_warm_block(Gi, Bi, Pn, 2, j1 - j0 - 1).cpu().numpy()          # a row range of the caller's table
            assert np.array_equal(_bits(part), _bits(A[j0 + 2:j1 - 1])), (j0, j1)
        if even:
            assert np.array_equal(_bits(aud), _bits(np.ascontiguousarray(S[:, j0:j1].T))), (j0, j1)
        else:
            gdev, allow = _report("audience_warm_block k=%d d=%d [%d, %d)" % (k, d, j0, j1), r64[:, j0:j1].T, r32[:, j0:j1].T, aud)
            assert gdev <= allow
            gdev, allow = _report("score_warm_block k=%d d=%d [%d, %d)" % (k, d, j0, j1), r64[:, j0:j1], r32[:, j0:j1], S[:, j0:j1])
            assert gdev <= allow
    if d:
        Fn_dev, _ = _proj(e, t["Fn"])
        n = int(Fn_dev.shape[0])
        zG, zB = torch.zeros((n, k), device="cuda"), torch.zeros(n, device="cuda")
        want = e.score_new_block(3, 290, Fn_dev).cpu().numpy()
        got = e.score_warm_block(3, 290, zG, zB, Fn_dev).cpu().numpy()
        if even:
            assert np.array_equal(_bits(got), _bits(want))
            assert np.array_equal(_bits(e.audience_warm_block(zG, zB, Fn_dev, 0, n).cpu().numpy()), _bits(e.audience_block(0, n, Fn_dev).cpu().numpy()))
        else:
            z64, z32 = (R.scores(t["Gu"], t["Tu"], zG.cpu().numpy(), zB.cpu().numpy(), Fn_dev.cpu().numpy(), dt)[3:290] for dt in (np.float64, np.float32))
            gdev, allow = _report("zero rows k=%d d=%d" % (k, d), z64, z32, got)
            assert gdev <= allow and float(np.abs(want - z64).max()) <= allow
    e.sync_check()
    e.close()


# ---- neutrality and lifecycle ----------------------------------------------------------------------------------------------------
def _warm_calls(e, Fn, seed=60):
    """fold_in_items, score_warm_block and audience_warm_block for 20 new items of a 300-user, 600-item engine."""
    from fashionvisualexpl_recommend_amd.models import draw_item_fold_pairs
    rs = np.random.RandomState(seed)
    train = [list(rs.choice(600, size=rs.randint(1, 9), replace=False)) for _ in range(300)]
    buyers = [list(rs.choice(300, size=rs.randint(0, 7), replace=False)) for _ in range(20)]
    ptr, user, other, role = draw_item_fold_pairs(buyers, train, 600, 3, seed=1)
    Pn = e.project_rows(Fn)
    Gi, Bi = torch.zeros((20, e.k), device="cuda"), torch.zeros(20, device="cuda")
    e.fold_in_items(ptr, user, other, role, 4, Gi, Bi, Pn, lr=0.05, reg=1e-3)
    assert Gi.abs().max() > 0
    return e.score_warm_block(0, 300, Gi, Bi, Pn), e.audience_warm_block(Gi, Bi, Pn, 0, 20)


@pytest.mark.parametrize("opt,form", [("sgd", None), ("adam_tf23", "lazy"), ("adam_tf23", "sweep")])
def test_the_calls_leave_the_state_alone(monkeypatch, opt, form):
    """Tables and Adam slots are bit-identical before and after the calls, and a 6-step run with them between steps 3 and 4 ends
    bit-identical to a run without them (duplicate-free batches: the step itself is then free of atomic-order noise)."""
    t = _tables(300, 600, 16, 12, 128, 100, "bf16", seed=17)
    Fn = _tables(20, 20, 16, 12, 128, 100, "bf16", seed=19)["F"]
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
                _warm_calls(e, Fn)
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
    t = C.tables(16, 12, seed=70)
    e = _engine(t)
    fp8 = _engine(dict(t, F=np.tile(t["F"], (1, 16)), E=np.tile(t["E"], (16, 1)), Bp=np.tile(t["Bp"], 16)), dtype="fp8")
    mf = _engine(C.tables(16, 0, seed=70))
    unbound = Engine(model="bprmf", num_users=8, num_items=I, embed_k=16, optimizer="sgd", max_batch=8)
    rs = np.random.RandomState(71)
    acf = _acf_engine(random_tables(rs, 6, 20, 16, 8, 4, 4), _acf_features(rs, 20, 2, 8, "fp32"), _acf_lists(rs, 6, 20, [2, 0, 3, 1, 2, 2]))
    Pn = e.project_rows(t["Fn"][:2])
    held = lib.bprx_live_device_allocs()
    i32 = lambda *v: torch.as_tensor(np.array(v, np.int32), device="cuda")
    ptr = torch.as_tensor(np.array([0, 2, 3], np.int64), device="cuda")
    user, other, role = i32(1, 2, 3), i32(4, 5, 6), i32(0, 1, 0)
    Gi, Bi, loss = torch.zeros((2, 16), device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    p = lambda x: None if x is None else x.data_ptr()

    def call(h, n=2, steps=1, opt=0, ptr_=ptr, user_=user, other_=other, role_=role, Pn_=Pn, Gi_=Gi, Bi_=Bi):
        return lib.bprx_fold_in_items(h, p(ptr_), p(user_), p(other_), p(role_), n, p(Pn_), steps, 0.05, 1e-3, opt, p(Gi_), p(Bi_),
                                      p(loss), None)

    assert call(e.h) == 0
    good = np.concatenate([Gi.cpu().numpy(), Bi.cpu().numpy()[:, None]], 1)
    assert np.abs(good[:, :16]).max() > 0 and np.abs(good[:, 16]).min() > 0
    assert call(e.h, n=0) == 0 and call(e.h, n=0, user_=None, other_=None, role_=None) == 0
    for kw in (dict(n=-1), dict(steps=0), dict(opt=2), dict(ptr_=None), dict(user_=None), dict(other_=None), dict(role_=None),
               dict(Pn_=None), dict(Gi_=None), dict(Bi_=None)):
        assert call(e.h, **kw) == _ffi.E_INVALID, kw
    assert call(mf.h) == _ffi.E_INVALID and call(mf.h, Pn_=None) == 0             # Pn is NULL iff d == 0
    assert call(acf.h, Pn_=None) == _ffi.E_INVALID
    assert call(fp8.h) == _ffi.E_INVALID and "fp8" in lib.bprx_last_error(fp8.h).decode()
    assert call(unbound.h, Pn_=None) == _ffi.E_STATE
    sc, au = torch.zeros((U, 2), device="cuda"), torch.zeros((2, U), device="cuda")
    warm = lambda h, u0=0, u1=U, G=Gi, B=Bi, P=Pn, n=2, out=sc: lib.bprx_score_warm_block(h, u0, u1, p(G), p(B), p(P), n, p(out), None)
    assert warm(e.h) == 0 and warm(e.h, u0=5, u1=5, G=None, B=None, P=None, out=None) == 0 and warm(e.h, n=0, G=None, B=None, P=None, out=None) == 0
    for kw in (dict(n=-1), dict(u0=-1), dict(u1=U + 1), dict(u0=2, u1=1), dict(G=None), dict(B=None), dict(P=None), dict(out=None)):
        assert warm(e.h, **kw) == _ffi.E_INVALID, kw
    assert warm(acf.h, P=None, u1=6) == _ffi.E_INVALID and warm(fp8.h) == _ffi.E_INVALID and warm(unbound.h, P=None, u1=8) == _ffi.E_STATE
    aud = lambda h, G=Gi, B=Bi, P=Pn, n=2, q0=0, q1=2, out=au: lib.bprx_audience_warm_block(h, p(G), p(B), p(P), n, q0, q1, p(out), None)
    assert aud(e.h) == 0 and aud(e.h, q0=1, q1=1, G=None, B=None, P=None, out=None) == 0
    for kw in (dict(n=-1), dict(q0=-1), dict(q1=3), dict(q0=2, q1=1), dict(G=None), dict(B=None), dict(P=None), dict(out=None)):
        assert aud(e.h, **kw) == _ffi.E_INVALID, kw
    assert aud(acf.h, P=None) == _ffi.E_INVALID and aud(fp8.h) == _ffi.E_INVALID and aud(unbound.h, P=None) == _ffi.E_STATE
    e.sync_check()
    # ids out of range and a role that is neither 0 nor 1: clamped, reported by sync_check (once); the handle goes on working
    for kw, clamp in ((dict(user_=i32(1, U, 3)), dict(user_=i32(1, U - 1, 3))), (dict(other_=i32(4, I, 6)), dict(other_=i32(4, I - 1, 6))),
                      (dict(other_=i32(4, -7, 6)), dict(other_=i32(4, 0, 6))), (dict(role_=i32(0, 2, 0)), dict(role_=i32(0, 1, 0))),
                      (dict(role_=i32(0, 1, -1)), dict(role_=i32(0, 1, 0)))):
        Gi.zero_(); Bi.zero_()
        assert call(e.h, **kw) == 0
        with pytest.raises(_ffi.BprxError) as err:
            e.sync_check()
        assert err.value.code == _ffi.E_RANGE
        clamped = Gi.cpu().numpy().copy()
        Gi.zero_(); Bi.zero_()
        assert call(e.h, **clamp) == 0
        e.sync_check()
        assert np.array_equal(_bits(clamped), _bits(Gi.cpu().numpy())), kw
    Gi.zero_(); Bi.zero_()
    assert call(e.h) == 0 and np.array_equal(_bits(good[:, :16]), _bits(Gi.cpu().numpy())) and np.array_equal(_bits(good[:, 16]), _bits(Bi.cpu().numpy()))
    e.sync_check()
    assert lib.bprx_live_device_allocs() == held                    # the calls allocated nothing
    del Pn
    for eng in (e, fp8, mf, unbound, acf):
        eng.close()
    assert lib.bprx_live_device_allocs() == live


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _model(rec, nu=130, Inum=60, **kw):
    from fashionvisualexpl_recommend_amd.models import BPRMF, VBPR
    p = dict(dataset="vb", validation=True, batch_size=64, epochs=1, batch_eval=128, embed_k=8, embed_d=6, lr=0.05, reg=1e-3,
             top_k=10, verbose=-1, restore_epochs=1, rec=rec, best_metric="ndcg", optimizer="adam_tf23", init_seed=5, dtype="fp32")
    p.update(kw)
    p = Namespace(**p)
    tr, va, te = synth.make_interactions(nu, Inum, per_user=8, seed=39)
    data = Namespace(num_users=nu, num_items=Inum, training_list=tr, validation_list=va, test_list=te, params=p)
    if rec == "bprmf":
        return BPRMF(data, p), tr, None
    raw = synth.make_features(Inum, 32, seed=40) * 3.7
    return VBPR(data, p, features=raw), tr, synth.make_features(25, 32, seed=41) * 3.0


@pytest.mark.parametrize("rec", ["bprmf", "vbpr"])
def test_recommend_warm_and_audience_warm_rank_as_the_float64_restatement(rec):
    """End to end on synth: fold_in_items -> score_warm_block / audience_warm_block -> topk_rows_masked against the restatement's
    ranking, wherever the score allowance rules out a near-tie around a list position; masked entries never appear."""
    from fashionvisualexpl_recommend_amd.models import draw_item_fold_pairs
    m, tr, raw = _model(rec)
    eng, nu, n, K = m.engine, 130, 25, 10
    rs = np.random.RandomState(42)
    buyers = [list(rs.choice(nu, size=c, replace=False)) for c in [0, 1, 2, 40] + list(rs.randint(1, 9, size=n - 4))]
    buyers[2] = buyers[2] + buyers[2][:1]                                # a buyer twice
    fold = dict(steps=6, negatives=3, seed=3, optimizer="sgd", lr=0.01)
    with pytest.raises(ValueError):
        m.fold_in_items(buyers, None if rec == "vbpr" else np.zeros((n, 4)), **fold)
    ids, vals = m.recommend_warm(buyers, raw, **fold)
    aid, aval = m.audience_warm(buyers, raw, k=K, **fold)
    assert ids.shape == vals.shape == (nu, K) and aid.shape == aval.shape == (n, K)
    Gi, Bi, Pn = m.fold_in_items(buyers, raw, **fold)
    assert (Pn is None) == (rec == "bprmf") and not Gi[0].any() and not Bi[0].any() and Gi[1:].abs().sum(1).min() > 0
    ptr, user, other, role = draw_item_fold_pairs(buyers, tr[:nu], 60, 3, seed=3)
    t = {nm: eng.t[nm].cpu().numpy() for nm in ("Gu", "Gi", "Bi") + (("Tu",) if eng.d else ())}
    P = eng.project_rows(eng.t["F"]).cpu().numpy()[:, :eng.d + 1] if eng.d else None
    Pn_h = Pn.cpu().numpy()[:, :eng.d + 1] if eng.d else None
    W0 = np.zeros((n, eng.k + 1), np.float32)
    hp = dict(steps=6, lr=0.01, reg=1e-3, optimizer="sgd")
    r64, r32 = (C.restate(t, P, Pn_h, ptr, user, other, role, W0, hp, dt) for dt in (np.float64, np.float32))
    gdev, allow = _report("model rows %s" % rec, C.rows(r64), C.rows(r32), C.rows((Gi.cpu().numpy(), Bi.cpu().numpy())))
    assert gdev <= allow
    S64 = R.scores(t["Gu"], t.get("Tu"), r64["Gi"], r64["Bi"], Pn_h)
    S32 = R.scores(t["Gu"], t.get("Tu"), r32["Gi"], r32["Bi"], Pn_h, np.float32)
    _, sallow = _allow(S64, S32)
    sc = eng.score_warm_block(0, nu, Gi, Bi, Pn)
    assert float(np.abs(sc.cpu().numpy() - S64).max()) <= sallow
    if rec == "vbpr":                                                    # the item without buyers: exactly the visual score
        assert np.array_equal(_bits(sc[:, 0].cpu().numpy()), _bits(eng.score_new_block(0, nu, Pn)[:, 0].cpu().numpy()))
    bought = [[j for j in range(n) if u in buyers[j]] for u in range(nu)]
    checked = 0
    for lists, got_ids, got_vals, S, masks in ((nu, ids, vals, S64, bought), (n, aid, aval, S64.T, buyers)):
        for r in range(lists):
            row = S[r].copy()
            row[masks[r]] = -np.inf
            order = np.argsort(-row, kind="stable")
            live = int(np.isfinite(row).sum())
            assert not set(got_ids[r][got_ids[r] >= 0].tolist()) & set(int(x) for x in masks[r]), r
            assert (got_ids[r] >= 0).sum() == min(K, live)
            top = min(K, live)
            gaps = row[order[:top]] - row[order[1:top + 1]]
            if (gaps <= 2 * sallow).any():
                continue
            assert np.array_equal(got_ids[r][:top], order[:top]), r
            assert np.abs(got_vals[r][:top] - row[order[:top]]).max() <= sallow
            checked += 1
    print("model %s: %d of %d lists ranked as float64" % (rec, checked, nu + n))
    assert checked >= (nu + n) // 2
    eng.sync_check()
    eng.close()


# ---- files -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", ["bprmf", "vbpr"])
def test_cli_writes_warm_files_next_to_unchanged_recommendations(tmp_path, rec):
    from fashionvisualexpl_recommend_amd import train_rec
    nu, Inum, top_k, n_new, K = 30, 60, 10, 7, 5
    tr, va, te = synth.make_interactions(nu, Inum, per_user=8, seed=53)
    synth.write_dataset(str(tmp_path), "toy", tr, va, te, Inum, features=synth.make_features(Inum, 32, seed=55) if rec == "vbpr" else None)
    new = []
    if rec == "vbpr":
        np.save(str(tmp_path / "new.npy"), synth.make_features(n_new, 32, seed=56) * 2.0)
        new = ["--new_items", str(tmp_path / "new.npy")]
    buyers = {0: [3, 9, 21], 2: [7], 5: [5, 6, 5]}                       # rows 1, 3, 4 (and 6 with --new_items) have no buyers
    rows = [(0, 3), (2, 7), (0, 9), (5, 5), (5, 6), (0, 21), (5, 5)]
    (tmp_path / "warm.tsv").write_text("".join("%d\t%d\n" % r for r in rows))
    n_warm = n_new if rec == "vbpr" else 6
    # --batch_size 1: a step adds at most one term to a gradient row, so runs of the same seed agree bit for bit
    common = ["--rec", rec, "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--reg", "0.01", "--top_k", str(top_k), "--lr", "0.01", "--optimizer", "sgd"] + new
    res = [str(tmp_path / ("res%d" % q)) for q in range(3)]
    warm = ["--warm_items", str(tmp_path / "warm.tsv"), "--fold_steps", "9", "--fold_negatives", "3"]
    train_rec.train(common + ["--results_root", res[0]])
    train_rec.train(common + ["--results_root", res[1]] + warm)
    train_rec.train(common + ["--results_root", res[2], "--audience", str(K)] + warm)
    (tmp_path / "stranger.tsv").write_text("0\t3\n1\t%d\n" % nu)
    with pytest.raises(ValueError, match="a buyer is outside the %d users" % nu):       # before anything is trained
        train_rec.train(common + ["--results_root", str(tmp_path / "res3"), "--warm_items", str(tmp_path / "stranger.tsv")])
    assert not os.path.exists(os.path.join(str(tmp_path / "res3"), "rec_results", "toy", rec)) or not os.listdir(os.path.join(str(tmp_path / "res3"), "rec_results", "toy", rec))
    rdir = [os.path.join(r, "rec_results", "toy", rec) for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] if "warm-" in f] and not [f for f in files[1] if "warm-audience" in f]
    assert [f for f in files[1] if "warm-" not in f] == files[0]
    for f in files[0]:                                                    # every other file: the bytes of the run without the flag
        assert open(os.path.join(rdir[0], f), "rb").read() == open(os.path.join(rdir[1], f), "rb").read(), f
    base = [f for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(base) == 2
    for f in base:
        assert open(os.path.join(rdir[0], f), "rb").read() == open(os.path.join(rdir[2], f), "rb").read(), f
        name = f.replace("recs-", "warm-recs-", 1)
        assert name in files[1] and name in files[2]
        assert open(os.path.join(rdir[1], name), "rb").read() == open(os.path.join(rdir[2], name), "rb").read()    # one fit serves both
        got = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], name))]
        assert all(len(r) == 3 for r in got)
        for u in range(nu):
            blk = [r for r in got if int(r[0]) == u]
            mine = {j for j, who in buyers.items() if u in who}
            assert len(blk) == min(top_k, n_warm - len(mine)) and not {int(r[1]) for r in blk} & mine
            sc = [float(r[2]) for r in blk]
            assert sc == sorted(sc, reverse=True) and len({r[1] for r in blk}) == len(blk)
            assert all(0 <= int(r[1]) < n_warm for r in blk)
        aud = f.replace("recs-", "warm-audience-", 1)
        assert aud in files[2]
        got = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[2], aud))]
        assert [int(r[0]) for r in got] == [j for j in range(n_warm) for _ in range(K)]
        for j in range(n_warm):
            blk = got[j * K:(j + 1) * K]
            sc = [float(r[2]) for r in blk]
            assert sc == sorted(sc, reverse=True) and not {int(r[1]) for r in blk} & set(buyers.get(j, []))
        if rec == "vbpr":                                                 # a row without buyers scores exactly as new-recs-* scores it
            vis = {(r[0], r[1]): r[2] for r in (l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], f.replace("recs-", "new-recs-", 1))))}
            cold = [r for r in (l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], name))) if int(r[1]) in (1, 3, 4, 6)]
            assert cold and all(vis[(r[0], r[1])] == r[2] for r in cold)
