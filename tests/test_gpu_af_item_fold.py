"""Warm items and audiences for AttentiveFashion on the MI355X, against the float64 restatement (tests/af_item_fold_ref.py):
bprx_af_encode_new, bprx_af_fold_in_items, bprx_af_score_warm_block, bprx_af_audience_block and the model methods and the CLI
flags on top of them.  Inputs: tests/af_item_fold_cases.py (checked on the CPU side by tests/test_af_item_fold_cpu.py).  The
restatement is fed the GPU's own encodings (af_encode, af_encode_new): the conv's kinks stay out of this test.

Allowance (the project's rule): 32 x the float32 restatement's max-abs deviation from float64 over the case, never below one
float32 ulp of the largest magnitude compared.  sgd leaves nothing out; Adam compares the entries af_item_fold_cases.adam_keep
keeps (at most 5 % left out).  Loss: 1e-5 relative.  Every check prints its triple (float32 deviation / allowance / GPU deviation).
What is exact is checked exactly."""
import gc
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import af_item_fold_cases as K
import af_item_fold_ref as R
from fashionvisualexpl_recommend_amd import _ffi

pytestmark = pytest.mark.gpu

I, U, BIG = K.I, K.U, K.BIG


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _engine(t, inputs, optimizer="sgd", lr=0.05, reg=1e-3, B=64, rate=0.5):
    from test_gpu_attentive import _engine as af_engine
    return af_engine(t, inputs, optimizer=optimizer, lr=lr, reg=reg, B=B, rate=rate)


def _fold(e, Cn, ptr, user, other, role, W0, want_work=False, **hp):
    """One bprx_af_fold_in_items call from the start rows W0: (Gi, loss[, work]) as numpy arrays."""
    Gi = torch.as_tensor(np.ascontiguousarray(W0), device="cuda")
    Cn = Cn if isinstance(Cn, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(Cn), device="cuda")
    out = e.af_fold_in_items(ptr, user, other, role, hp["steps"], Cn, Gi, lr=hp["lr"], reg=hp["reg"], optimizer=hp["optimizer"],
                             want_work=want_work)
    if want_work:
        return Gi.cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy()
    return Gi.cpu().numpy(), out.cpu().numpy()


def _sub(Cn, ptr, user, other, role, W0, items):
    """The call for the listed items only, in the listed order."""
    items = list(items)
    cnt = [int(ptr[r + 1] - ptr[r]) for r in items]
    p = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in items] + [np.zeros(0, np.int64)]).astype(np.int64)
    return np.ascontiguousarray(Cn[:, items]), p, user[take], other[take], role[take], W0[items]


def _allow(d32, ref):
    return max(32.0 * d32, float(np.spacing(np.float32(np.abs(ref).max()))))


_cache = {}


def _case(k, h):
    """The host case of one width, its engine, the GPU's encodings, the restatements on them (float64, float32; sgd and adam; the
    WIDE shapes sgd only) and the GPU's results of the whole call: made once, never changed."""
    if (k, h) not in _cache:
        c = dict(K.case(k, h))
        e = _engine(c["t"], c["inputs"])
        c["e"] = e
        c["Cg"] = e.af_encode(np.arange(I)).cpu().numpy()
        c["Cng_dev"] = e.af_encode_new(*c["new"])
        c["Cng"] = c["Cng_dev"].cpu().numpy()
        args = (c["t"], c["Cg"], c["Cng"], c["ptr"], c["user"], c["other"], c["role"], c["W0"])
        for name, hp in (("sgd", K.SGD),) + ((("adam", K.ADAM),) if (k, h) in K.WIDTHS else ()):
            c[name + "64"], c[name + "32"] = K.restate(*args, hp), K.restate(*args, hp, np.float32)
            c[name + "_gpu"] = _fold(e, c["Cng_dev"], *args[3:], want_work=True, **hp)
        e.sync_check()
        _cache[(k, h)] = c
    return _cache[(k, h)]


def _check(tag, hp, c, r64, r32, got, loss):
    has = np.diff(c["ptr"]) > 0
    dev32 = np.abs(r32["Gi"].astype(np.float64) - r64["Gi"])
    gdev = np.abs(got.astype(np.float64) - r64["Gi"])
    left = 0.0
    if hp["optimizer"] != "sgd":
        keep, left = K.adam_keep(r64, c["ptr"])
        dev32, gdev = np.where(keep, dev32, 0.0), np.where(keep, gdev, 0.0)
    allow = _allow(float(dev32.max()), r64["Gi"])
    err = np.abs(loss.astype(np.float64) - r64["loss"])
    print("%s: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e; left out %.2f %%; loss relative error up to %.3e" % (
        tag, dev32.max(), allow, gdev.max(), 100 * left, (err[has] / np.abs(r64["loss"][has])).max()))
    assert left <= 0.05
    assert np.isfinite(got).all() and gdev.max() <= allow, (tag, gdev.max(), allow)
    assert (err <= 1e-5 * np.abs(r64["loss"])).all(), (tag, np.nonzero(err > 1e-5 * np.abs(r64["loss"]))[0])
    assert loss[0] == 0 and np.array_equal(_bits(got[0]), _bits(c["W0"][0]))      # no pairs: the row stays, loss 0


def _check_scores(tag, Gu, att, C, Gi, x, al):
    """Scores and attentions against the float64 restatement, the allowance from the float32 one."""
    (x64, a64), (x32, a32) = R.scores(Gu, att, C, Gi), R.scores(Gu, att, C, Gi, np.float32)
    for what, got, r64, r32 in (("scores", x, x64, x32), ("alpha", al, a64, a32)):
        d32 = float(np.abs(r32 - r64).max())
        allow, gdev = _allow(d32, r64), float(np.abs(got - r64).max())
        print("%s %s: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (tag, what, d32, allow, gdev))
        assert gdev <= allow, (tag, what)


# ---- against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,h", K.WIDTHS)
def test_work_rows_against_float64(k, h):
    """work row p = [D_p (k) | dc_p | zeros]; item 6's pairs 4 and 5 are one (u, o) in both roles: bit negations of each other."""
    c = _case(k, h)
    work = c["sgd_gpu"][2]
    KW = (k + 1 + 3) // 4 * 4
    assert work.shape == (c["ptr"][-1], KW) and c["e"].af_work_stride() == KW
    D64, dc64 = np.concatenate(c["sgd64"]["D"]), np.concatenate(c["sgd64"]["dc"])
    D32, dc32 = np.concatenate(c["sgd32"]["D"]), np.concatenate(c["sgd32"]["dc"])
    d32 = max(float(np.abs(D32 - D64).max()), float(np.abs(dc32 - dc64).max()))
    allow = _allow(d32, np.concatenate([D64.reshape(-1), dc64]))
    gdev = max(float(np.abs(work[:, :k] - D64).max()), float(np.abs(work[:, k] - dc64).max()))
    print("work k=%d h=%d: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (k, h, d32, allow, gdev))
    assert gdev <= allow
    assert not work[:, k + 1:].any()                                              # the padding is zero
    p = int(c["ptr"][6]) + 4
    assert c["role"][p] != c["role"][p + 1] and c["user"][p] == c["user"][p + 1] and c["other"][p] == c["other"][p + 1]
    assert np.array_equal(_bits(work[p, :k + 1]) ^ np.int32(-2 ** 31), _bits(work[p + 1, :k + 1]))
    assert np.abs(work[p, :k + 1]).min() > 0
    assert np.array_equal(_bits(work), _bits(c["adam_gpu"][2]))                   # the pair terms do not depend on the fit


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("k,h", K.WIDTHS)
def test_rows_and_loss_against_float64(k, h, opt):
    c = _case(k, h)
    got, loss = c[opt + "_gpu"][:2]
    _check("%s k=%d h=%d" % (opt, k, h), K.SGD if opt == "sgd" else K.ADAM, c, c[opt + "64"], c[opt + "32"], got, loss)


@pytest.mark.parametrize("k,h", K.WIDE)
def test_wide_rows(k, h):
    """Near the bind limit (k x 32 <= 15 360): eight lane words per row, 60 KB of LDS in the pair kernel, two pairs per group."""
    c = _case(k, h)
    got, loss = c["sgd_gpu"][:2]
    _check("sgd k=%d h=%d" % (k, h), K.SGD, c, c["sgd64"], c["sgd32"], got, loss)
    args = (c["Cng"], c["ptr"], c["user"], c["other"], c["role"], c["W0"])
    again = _fold(c["e"], *args, **K.SGD)
    assert np.array_equal(_bits(got), _bits(again[0])) and np.array_equal(_bits(loss), _bits(again[1]))
    part = _fold(c["e"], *_sub(*args, [7, 0, 4]), **K.SGD)
    assert np.array_equal(_bits(part[0]), _bits(got[[7, 0, 4]])) and np.array_equal(_bits(part[1]), _bits(loss[[7, 0, 4]]))
    c["e"].sync_check()


# ---- bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,h", K.WIDTHS)
def test_an_items_bits_depend_on_nothing_but_the_item(monkeypatch, k, h):
    c = _case(k, h)
    e = c["e"]
    args = (c["Cng"], c["ptr"], c["user"], c["other"], c["role"], c["W0"])
    for name, hp in (("sgd", K.SGD), ("adam", K.ADAM)):
        rows, loss = c[name + "_gpu"][:2]
        again = _fold(e, *args, **hp)
        assert np.array_equal(_bits(rows), _bits(again[0])) and np.array_equal(_bits(loss), _bits(again[1])), "two calls"
        perm = np.random.RandomState(7).permutation(K.N_NEW)
        shuffled = _fold(e, *_sub(*args, perm), **hp)
        assert np.array_equal(_bits(shuffled[0]), _bits(rows[perm])) and np.array_equal(_bits(shuffled[1]), _bits(loss[perm]))
        for items in ([0], [1], [BIG], [8], [129], range(4), range(5), [BIG, 0, 6, 7]):       # n = 1, 4, 5
            items = list(items)
            part = _fold(e, *_sub(*args, items), **hp)
            assert np.array_equal(_bits(part[0]), _bits(rows[items])), (name, items)
            assert np.array_equal(_bits(part[1]), _bits(loss[items])), (name, items)
    monkeypatch.setenv("BPRX_FOLD_CACHE", "0")                                    # read at create: every step reads work again
    e0 = _engine(c["t"], c["inputs"])
    for name, hp in (("sgd", K.SGD), ("adam", K.ADAM)):
        plain = _fold(e0, *args, **hp)
        assert np.array_equal(_bits(plain[0]), _bits(c[name + "_gpu"][0])), name
        assert np.array_equal(_bits(plain[1]), _bits(c[name + "_gpu"][1])), name
    e0.sync_check()
    e0.close()


@pytest.mark.parametrize("k,h", [(16, 32), (64, 64)])
def test_encode_new_is_encode_for_copies_of_catalogue_inputs(k, h):
    """300 rows are past one encode chunk (2 x max_batch = 128 rows)."""
    c = _case(k, h)
    e = c["e"]
    want = e.af_encode(np.arange(I))
    assert torch.equal(want.view(torch.int32), e.af_encode_new(*c["inputs"]).view(torch.int32))
    pick = np.random.RandomState(3).permutation(I)[:150]
    got = e.af_encode_new(*(np.ascontiguousarray(x[pick]) for x in c["inputs"]))
    assert torch.equal(want[:, torch.as_tensor(pick, device="cuda")].contiguous().view(torch.int32), got.view(torch.int32))
    assert tuple(e.af_encode_new(*(x[:0] for x in c["inputs"])).shape) == (3, 0, k)
    with pytest.raises(ValueError):
        e.af_encode_new(c["inputs"][0], c["inputs"][1][:, :5], c["inputs"][2])
    e.sync_check()


@pytest.mark.parametrize("k,h", [(5, 7), (16, 32), (64, 64), (20, 96)])
def test_warm_and_audience_blocks_are_score_block_for_catalogue_slices(k, h):
    """Rows sliced out of af_encode and Gi: the bits of those columns of af_score_block; item-major: the transposed bits, in the
    catalogue form and the caller-row form, for q ranges that start and end inside a 128-item tile, with and without alpha."""
    c = _case(k, h)
    e = c["e"]
    Call = e.af_encode(np.arange(I))
    eq = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    full_x, full_a = e.af_score_block(0, U)
    for (u0, u1), (i0, i1) in (((0, U), (0, I)), ((3, 4), (130, 131)), ((17, 150), (5, 200)), ((290, 300), (100, 300))):
        Cs, Gs = Call[:, i0:i1].contiguous(), e.t["Gi"][i0:i1].contiguous()
        x, al = e.af_score_warm_block(u0, u1, Cs, Gs)
        assert eq(x, full_x[u0:u1, i0:i1]) and eq(al, full_a[u0:u1, i0:i1]), (u0, u1, i0, i1)
        only, none = e.af_score_warm_block(u0, u1, Cs, Gs, want_alpha=False)
        assert none is None and eq(only, x)
    for q0, q1 in ((0, I), (3, 77), (130, 131), (100, 300), (127, 129)):
        x, al = e.af_audience_block(q0, q1)
        assert eq(x, full_x[:, q0:q1].T) and eq(al, full_a[:, q0:q1].transpose(0, 1)), (q0, q1)
        only, none = e.af_audience_block(q0, q1, want_alpha=False)
        assert none is None and eq(only, x)
    Cs, Gs = Call[:, 40:240].contiguous(), e.t["Gi"][40:240].contiguous()          # caller rows: row r is item 40 + r
    wx, wa = e.af_score_warm_block(0, U, Cs, Gs)
    for q0, q1 in ((0, 200), (7, 8), (90, 135), (129, 200)):
        x, al = e.af_audience_block(q0, q1, Cs, Gs)
        assert eq(x, wx[:, q0:q1].T) and eq(al, wa[:, q0:q1].transpose(0, 1)), (q0, q1)
        assert eq(x, full_x[:, 40 + q0:40 + q1].T)
        assert eq(e.af_audience_block(q0, q1, Cs, Gs, want_alpha=False)[0], x)
    # and against the restatement
    _check_scores("block k=%d h=%d" % (k, h), c["t"]["Gu"], K.att(c["t"]), c["Cg"], c["t"]["Gi"], full_x.cpu().numpy(), full_a.cpu().numpy())
    e.sync_check()


# ---- behaviour -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,h", [(16, 32), (64, 64)])
def test_one_sgd_step_moves_a_catalogue_items_row_as_bprx_step_does(k, h):
    """steps = 1, sgd, from catalogue item r's own Gi row and encodings on a handle bound with dropout = 0, against bprx_step on
    the batch that has the item once per triplet, in either role, on a second handle with identical tables."""
    c = K.case(k, h)
    t, inputs = c["t"], c["inputs"]
    rs = np.random.RandomState(41)
    r, B, lr, reg = 11, 37, 0.05, 1e-3
    user = rs.randint(U, size=B).astype(np.int32)
    other = rs.choice([i for i in range(I) if i != r], size=B).astype(np.int32)
    role = rs.randint(2, size=B).astype(np.int32)
    user[3], other[3], role[3] = user[2], other[2], role[2]                       # a pair twice
    ea, eb = (_engine(t, inputs, lr=lr, reg=reg, B=64, rate=0.0) for _ in range(2))
    C = ea.af_encode(np.arange(I)).cpu().numpy()
    hp = dict(steps=1, lr=lr, reg=reg, optimizer="sgd")
    G0 = t["Gi"][r:r + 1]
    Cn = np.ascontiguousarray(C[:, r:r + 1])
    fold = _fold(ea, Cn, [0, B], user, other, role, G0, **hp)[0][0]
    r64, r32 = (K.restate(t, C, Cn, [0, B], user, other, role, G0, hp, dt)["Gi"][0] for dt in (np.float64, np.float32))
    dev = lambda x: torch.as_tensor(x, device="cuda")
    pos, neg = np.where(role == 0, r, other).astype(np.int32), np.where(role == 0, other, r).astype(np.int32)
    eb.step(dev(user), dev(pos), dev(neg))
    stepped = eb.t["Gi"][r].cpu().numpy()
    d32 = float(np.abs(r32 - r64).max())
    allow = _allow(d32, r64)
    gap = float(np.abs(stepped.astype(np.float64) - fold).max())
    print("T=1 k=%d h=%d: float32 deviation %.3e / allowance %.3e / fold - float64 %.3e / bprx_step - float64 %.3e / bprx_step - "
          "fold %.3e" % (k, h, d32, allow, np.abs(fold - r64).max(), np.abs(stepped - r64).max(), gap))
    assert np.abs(stepped - G0[0]).max() > 1e-3                                   # (the step moved the row)
    assert gap <= allow
    for e in (ea, eb):
        e.sync_check()
        e.close()


def test_a_step_between_two_fits_is_seen_by_the_second():
    k, h = 16, 32
    c = K.case(k, h)
    e = _engine(c["t"], c["inputs"], lr=0.2, reg=1e-3, B=64, rate=0.0)
    items = [0, 1, 2, 5, 6, 7, 20, 21]
    Cn = e.af_encode_new(*c["new"]).cpu().numpy()
    args = _sub(Cn, c["ptr"], c["user"], c["other"], c["role"], c["W0"], items)
    first = _fold(e, *args, **K.SGD)[0]
    rs = np.random.RandomState(78)
    dev = lambda x: torch.as_tensor(x, device="cuda")
    e.step(dev(rs.randint(0, U, 64).astype(np.int32)), dev(rs.randint(0, I, 64).astype(np.int32)), dev(rs.randint(0, I, 64).astype(np.int32)))
    Cn2 = e.af_encode_new(*c["new"]).cpu().numpy()
    args2 = (np.ascontiguousarray(Cn2[:, items]),) + args[1:]
    second, loss = _fold(e, *args2, **K.SGD)
    assert not np.array_equal(_bits(first), _bits(second))                        # (the step moved what the fit reads)
    t2 = dict(c["t"])
    t2.update({n: v.cpu().numpy() for n, v in e.t.items() if n in ("Gu", "Gi") + R.ATT})
    C2 = e.af_encode(np.arange(I)).cpu().numpy()
    r64, r32 = (K.restate(t2, C2, *args2, K.SGD, dt) for dt in (np.float64, np.float32))
    d32 = float(np.abs(r32["Gi"] - r64["Gi"]).max())
    allow, gdev = _allow(d32, r64["Gi"]), float(np.abs(second - r64["Gi"]).max())
    print("fit / step / fit: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (d32, allow, gdev))
    assert gdev <= allow
    assert (np.abs(loss - r64["loss"]) <= 1e-5 * np.abs(r64["loss"])).all()
    e.sync_check()
    e.close()


def test_errors_leave_the_handle_usable_and_no_allocation_behind():
    from fashionvisualexpl_recommend_amd.engine import Engine
    lib = _ffi.lib()
    gc.collect()
    live = lib.bprx_live_device_allocs()
    k, h = 16, 32
    c = K.case(k, h)
    t = c["t"]
    e = _engine(t, c["inputs"])
    plain = Engine(model="bprmf", num_users=U, num_items=I, embed_k=k, optimizer="sgd", max_batch=8).bind(t["Gu"], t["Gi"], t["Bi"])
    unbound = Engine(model="bprmf", num_users=U, num_items=I, embed_k=k, optimizer="sgd", max_batch=8)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    n, KW = 3, 20
    ptr = dev(np.array([0, 2, 2, 3], np.int64))
    user, other, role = dev(np.array([1, 2, 3], np.int32)), dev(np.array([4, 5, 6], np.int32)), dev(np.array([0, 1, 0], np.int32))
    ed, col, cl = (dev(np.ascontiguousarray(x[:n])) for x in c["new"])
    Cn, Gi, loss, work = (torch.zeros(s, device="cuda") for s in ((3, n, k), (n, k), (n,), (3, KW)))
    sc, al = torch.zeros((2, n), device="cuda"), torch.zeros((2, n, 3), device="cuda")
    asc, aal = torch.zeros((n, U), device="cuda"), torch.zeros((n, U, 3), device="cuda")
    p = lambda x: None if x is None else x.data_ptr()

    def enc(hd, n_=n, ed_=ed, col_=col, cl_=cl, out_=Cn):
        return lib.bprx_af_encode_new(hd, p(ed_), p(col_), p(cl_), n_, p(out_), None)

    def fit(hd, n_=n, steps=1, opt=0, ptr_=ptr, user_=user, other_=other, role_=role, Cn_=Cn, Gi_=Gi, loss_=loss, work_=work):
        return lib.bprx_af_fold_in_items(hd, p(ptr_), p(user_), p(other_), p(role_), n_, p(Cn_), steps, 0.05, 1e-3, opt, p(Gi_), p(loss_),
                                         p(work_), None)

    def warm(hd, u0=0, u1=2, Cn_=Cn, Gi_=Gi, n_=n, out=sc, a=al):
        return lib.bprx_af_score_warm_block(hd, u0, u1, p(Cn_), p(Gi_), n_, p(out), p(a), None)

    def aud(hd, Cn_=Cn, Gi_=Gi, n_=n, q0=0, q1=n, out=asc, a=aal):
        return lib.bprx_af_audience_block(hd, p(Cn_), p(Gi_), n_, q0, q1, p(out), p(a), None)

    assert enc(e.h) == 0 and fit(e.h) == 0 and warm(e.h) == 0 and aud(e.h) == 0   # (the first fit: the catalogue encodings are made)
    torch.cuda.synchronize()
    held = lib.bprx_live_device_allocs()
    good = Gi.cpu().numpy().copy()
    assert np.abs(good[0]).max() > 0 and not good[1].any()
    Gi.zero_()
    assert fit(e.h, loss_=None) == 0 and np.array_equal(_bits(good), _bits(Gi))   # loss is optional
    before = [x.clone() for x in (Cn, Gi, sc, asc)]
    assert enc(e.h, n_=0) == 0 and fit(e.h, n_=0) == 0 and warm(e.h, n_=0) == 0 and warm(e.h, u0=1, u1=1) == 0 and aud(e.h, q0=2, q1=2) == 0
    assert all(torch.equal(a, b) for a, b in zip(before, (Cn, Gi, sc, asc)))      # nothing is written
    for kw in (dict(n_=-1), dict(ed_=None), dict(col_=None), dict(cl_=None), dict(out_=None)):
        assert enc(e.h, **kw) == _ffi.E_INVALID, kw
    for kw in (dict(n_=-1), dict(steps=0), dict(opt=2), dict(ptr_=None), dict(user_=None), dict(other_=None), dict(role_=None),
               dict(Cn_=None), dict(Gi_=None), dict(work_=None)):
        assert fit(e.h, **kw) == _ffi.E_INVALID, kw
    for kw in (dict(u0=-1), dict(u1=U + 1), dict(u0=2, u1=1), dict(n_=-1), dict(Cn_=None), dict(Gi_=None), dict(out=None)):
        assert warm(e.h, **kw) == _ffi.E_INVALID, kw
    for kw in (dict(q0=-1), dict(q1=n + 1), dict(q0=2, q1=1), dict(Cn_=None), dict(Gi_=None), dict(out=None), dict(Cn_=None, Gi_=None)):
        assert aud(e.h, **kw) == _ffi.E_INVALID, kw                                # (both NULL: the catalogue form takes n = num_items)
    for f in (enc, fit, warm, aud):
        assert f(plain.h) == _ffi.E_INVALID and "bprx_bind_attentive" in lib.bprx_last_error(plain.h).decode()
        assert f(unbound.h) == _ffi.E_STATE
    # the pinned rejections of the plain calls stay
    Bi = torch.zeros(n, device="cuda")
    assert lib.bprx_fold_in_items(e.h, p(ptr), p(user), p(other), p(role), n, None, 1, 0.05, 1e-3, 0, p(Gi), p(Bi), p(loss), None) == _ffi.E_INVALID
    assert lib.bprx_audience_block(e.h, None, I, 0, 1, p(asc), None) == _ffi.E_INVALID
    e.sync_check()
    # ids out of range: clamped, and reported by sync_check (once); the handle goes on working
    Gi.zero_()
    assert fit(e.h, user_=dev(np.array([1, U, 3], np.int32))) == 0
    with pytest.raises(_ffi.BprxError) as err:
        e.sync_check()
    assert err.value.code == _ffi.E_RANGE
    e.sync_check()                                                   # reported once
    clamped = Gi.cpu().numpy().copy()
    Gi.zero_()
    assert fit(e.h, user_=dev(np.array([1, U - 1, 3], np.int32))) == 0 and np.array_equal(_bits(clamped), _bits(Gi))
    for kw in (dict(other_=dev(np.array([4, -7, 6], np.int32))), dict(role_=dev(np.array([0, 2, 0], np.int32)))):
        Gi.zero_()
        assert fit(e.h, **kw) == 0
        with pytest.raises(_ffi.BprxError):
            e.sync_check()
    Gi.zero_()
    assert fit(e.h) == 0 and np.array_equal(_bits(good), _bits(Gi))
    e.sync_check()
    assert lib.bprx_live_device_allocs() == held                     # the calls allocated nothing
    for eng in (e, plain, unbound):
        eng.close()
    assert lib.bprx_live_device_allocs() == live


# ---- the model and the files ---------------------------------------------------------------------------------------------------
def _toy_model(tmp_path, **over):
    from fashionvisualexpl_recommend_amd import configs, models
    from test_gpu_attentive import _toy
    root, train, val, test = _toy(tmp_path)
    configs.set_roots(root, str(tmp_path / "res"))
    try:
        data = Namespace(num_users=40, num_items=24, training_list=train, validation_list=val, test_list=test,
                         params=Namespace(batch_eval=128))
        p = dict(epochs=1, batch_size=16, embed_k=16, lr=0.05, reg=1e-3, top_k=5, dataset="toy", rec="attentive_fashion",
                 attention_layers=[32, 1], dropout=0.5, optimizer="sgd", dtype="fp32")
        p.update(over)
        m = models.AttentiveFashion(data, Namespace(**p))
    finally:
        configs.set_roots("../data", "../results")
    return m, train


def _new_inputs(n, Dc=24, Dk=10, seed=9):
    from attentive_ref import random_inputs
    ed, col, cl = random_inputs(np.random.RandomState(seed), n, Dc, Dk)
    return ed, (col * 37.0).astype(np.float32), cl                  # raw histograms: the model divides by each row's max-abs


def test_warm_lists_mask_buyers_and_match_numpy(tmp_path):
    m, train = _toy_model(tmp_path, af_audience=7)
    Un, In, K5 = 40, 24, 5
    buyers = [[3, 7, 3, 11], [], [0, 1, 2], list(range(35)), [39], [5, 6], [8], [20, 21, 22, 23]]
    feats = _new_inputs(len(buyers))
    fold = dict(steps=6, negatives=3, seed=3)
    Gi, Cn = m.fold_in_items(buyers, feats, **fold)
    assert tuple(Gi.shape) == (8, 16) and tuple(Cn.shape) == (3, 8, 16) and not Gi[1].any() and Gi[[0, 2, 3]].abs().amax(1).min().item() > 0
    prepared = m.prepare_new_items(*feats)
    assert torch.equal(Cn, m.engine.af_encode_new(*prepared))
    sc, al = (v.cpu().numpy() for v in m.engine.af_score_warm_block(0, Un, Cn, Gi))
    _check_scores("warm block", m.engine.t["Gu"].cpu().numpy(), tuple(m.engine.t[n].cpu().numpy() for n in R.ATT), Cn.cpu().numpy(),
                  Gi.cpu().numpy(), sc, al)
    assert not sc[:, 1].any()                                        # a row without buyers scores 0.0 for everyone
    ids, vals, att = m.recommend_warm(buyers, feats, **fold)
    assert ids.shape == vals.shape == (Un, K5) and att.shape == (Un, K5, 3)
    for u in range(Un):
        mine = [j for j, who in enumerate(buyers) if u in who]
        row = sc[u].copy()
        row[mine] = -np.inf
        want = np.argsort(-row, kind="stable")[:K5]
        live = ids[u] >= 0
        assert not set(ids[u][live].tolist()) & set(mine), u
        assert np.array_equal(np.sort(vals[u])[::-1], vals[u]) and np.array_equal(_bits(vals[u]), _bits(row[want])), u
        assert np.array_equal(_bits(vals[u][live]), _bits(sc[u][ids[u][live]])) and np.array_equal(_bits(att[u][live]), _bits(al[u][ids[u][live]]))
    aid, aval, aatt = m.audience_warm(buyers, feats, **fold)
    tx, ta = (v.cpu().numpy() for v in m.engine.af_audience_block(0, 8, Cn, Gi))
    assert aid.shape == (8, 7) and np.array_equal(_bits(tx), _bits(sc.T))
    for j in range(8):
        row = tx[j].copy()
        row[buyers[j]] = -np.inf
        live = aid[j] >= 0
        assert live.sum() == min(7, Un - len(set(buyers[j]))) and not set(aid[j][live].tolist()) & set(buyers[j]), j
        assert np.array_equal(_bits(aval[j]), _bits(np.sort(row)[::-1][:7])), j
        assert np.array_equal(_bits(aatt[j][live]), _bits(ta[j][aid[j][live]]))
    assert (aid[3] >= 0).sum() == 5                                  # 35 of 40 users bought item 3
    cid, cval, catt = m.audience()
    cx, ca = (v.cpu().numpy() for v in m.engine.af_audience_block(0, In))
    for i in range(In):
        own = [u for u in range(Un) if i in train[u]]
        row = cx[i].copy()
        row[own] = -np.inf
        live = cid[i] >= 0
        assert not set(cid[i][live].tolist()) & set(own) and np.array_equal(_bits(cval[i]), _bits(np.sort(row)[::-1][:7])), i
        assert np.array_equal(_bits(catt[i][live]), _bits(ca[i][cid[i][live]]))
    m.engine.sync_check()
    m.engine.close()


def test_cli_writes_the_three_files(tmp_path):
    from fashionvisualexpl_recommend_amd import train_rec
    from test_gpu_attentive import _toy
    root, train, val, test = _toy(tmp_path)
    res, top_k, Kaud = str(tmp_path / "res"), 5, 6
    buyers = [[3, 7, 3], [], [0, 1, 2, 9], [39], [5, 6], [8, 30], [20]]
    paths = [str(tmp_path / n) for n in ("edges.npy", "colour.npy", "classes.npy")]
    for pth, a in zip(paths, _new_inputs(len(buyers))):
        np.save(pth, a)
    (tmp_path / "warm.tsv").write_text("".join("%d\t%d\n" % (j, u) for j, who in enumerate(buyers) for u in who))
    train_rec.train(["--rec", "attentive_fashion", "--dataset", "toy", "--data_root", root, "--results_root", res, "--epochs", "2",
                     "--batch_size", "32", "--embed_k", "16", "--attention_layers", "32", "1", "--reg", "0.01", "--top_k", str(top_k),
                     "--af_new_items"] + paths + ["--af_warm_items", str(tmp_path / "warm.tsv"), "--af_audience", str(Kaud),
                                                  "--fold_steps", "9", "--fold_negatives", "3"])
    rdir = os.path.join(res, "rec_results", "toy", "attentive_fashion")
    files = sorted(os.listdir(rdir))
    base = [f for f in files if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(base) == 2
    for f in base:
        read = lambda kind: [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir, f.replace("recs-", kind + "-", 1)))]
        recs, waud, aud = read("warm-recs"), read("warm-audience"), read("audience")
        for rows in (recs, waud, aud):
            assert all(len(r) == 6 for r in rows)                    # label  id  score  alpha_colour  alpha_edges  alpha_class
            assert max(abs(sum(float(v) for v in r[3:]) - 1.0) for r in rows) <= 1e-6
        bought = {u: {j for j, who in enumerate(buyers) if u in who} for u in range(40)}
        assert len(recs) == sum(min(top_k, len(buyers) - len(bought[u])) for u in range(40))
        assert all(int(r[1]) not in bought[int(r[0])] for r in recs)
        assert len(waud) == len(buyers) * Kaud and all(int(r[1]) not in buyers[int(r[0])] for r in waud)
        assert all(float(r[2]) == 0.0 for r in waud if r[0] == "1") and all(float(r[2]) == 0.0 for r in recs if r[1] == "1")
        assert len(aud) == 24 * Kaud and all(int(r[0]) not in train[int(r[1])] for r in aud)
        for rows in (recs, waud, aud):
            for lab in {r[0] for r in rows}:
                s = [float(r[2]) for r in rows if r[0] == lab]
                assert s == sorted(s, reverse=True), lab
