"""Calibrated lists on the MI355X: bprx_calibrate against the float64 restatement (tests/calibrate_ref.py), the model methods on top
of it and the cal-* files of train_rec --calibrate.

A greedy choice is discontinuous, so list identities are never compared across precisions and no near-tie is left out: the GPU's
OWN list is replayed in float64.  At each step, given the GPU's prefix, the float64 objective of the GPU's pick must lie within
the allowance of the largest float64 objective among the remaining candidates, and the GPU's gain within the allowance of the
float64 one; the same for both kl values; val is bit-equal to the pool's score at the returned id, cls is the table's entry.

Allowance per compared output (the rule of tests/test_gpu_diversify.py, _allowance): 32 x the max-abs deviation of the FLOAT32
restatement (replaying the same list) from the float64 one over the case, never below one float32 ulp of the output's largest
magnitude.  Every comparison prints its triple (float32 deviation / allowance / GPU deviation).  What is exact is checked exactly."""
import gc
import io
import os

import numpy as np
import pytest
import torch

import calibrate_ref as R
from fashionvisualexpl_recommend_amd import _ffi, ranking, synth
from test_gpu_diversify import _allowance, _pools, _positions
from test_gpu_feat_explain import _bits, _snapshot, _tables, _unique_batches, _vbpr
from test_gpu_new_items import GUARD, PATTERN, _model
from test_gpu_similar import _bprmf

pytestmark = pytest.mark.gpu

NS = (1, 20, 63, 64, 65, 70, 256)
CS = (1, 2, 7, 255, 256, 257, 1024)
MIX = ((0.0, 0.01), (0.5, 0.01), (0.99, 0.5), (1.0, 0.01), (0.5, 0.5))       # (lambda, alpha): every lambda, both alphas
_ENGINE = {}


def _handle():
    """One small bound BPRMF handle for the calls of this file: the entry reads no model table."""
    if "e" not in _ENGINE:
        _ENGINE["e"] = _bprmf(_tables(8, 16, 4, 4, 16, 8, "fp32", seed=1))
    return _ENGINE["e"]


def _table(I, C, seed):
    """The class of every item: every class id up to C - 1 where the catalogue is large enough, about a seventh without a class."""
    rs = np.random.RandomState(seed)
    t = rs.randint(0, C, I)
    t[rs.permutation(I)[:min(I, C)]] = np.arange(min(I, C))
    t[rs.rand(I) < 0.15] = -1
    t[:3] = (-1, C - 1, 0)
    return t.astype(np.int32)


def _hists(n, I, table, seed):
    """n histories, by row modulo 7: empty, one entry, all classless, one class only, 700 entries (more than a workgroup has
    threads), ids outside [0, I) mixed in, a short random one."""
    rs = np.random.RandomState(seed)
    none, some = np.flatnonzero(table < 0), np.flatnonzero(table >= 0)
    out = []
    for r in range(n):
        kind = r % 7
        if kind == 0:
            h = []
        elif kind == 1:
            h = [int(some[rs.randint(some.size)])]
        elif kind == 2:
            h = none[rs.randint(none.size, size=9)].tolist()
        elif kind == 3:
            c = table[some[rs.randint(some.size)]]
            h = rs.choice(np.flatnonzero(table == c), 6).tolist()
        elif kind == 4:
            h = rs.randint(0, I, 700).tolist()
        elif kind == 5:
            h = rs.randint(0, I, 30).tolist() + [-1, -7, I, I + 5, 2 ** 31 - 1, -2 ** 31]
            rs.shuffle(h)
        else:
            h = rs.randint(0, I, rs.randint(2, 25)).tolist()
        out.append(h)
    return out


def _csr(hists):
    ptr = np.zeros(len(hists) + 1, np.int64)
    np.cumsum([len(h) for h in hists], out=ptr[1:])
    items = np.array([i for h in hists for i in h] or [0], np.int32)
    return torch.as_tensor(ptr, device="cuda"), torch.as_tensor(items, device="cuda")


def _call(e, ids, vals, csr, table, C, K, lam, alpha, row0=0, want_kl=True):
    """One bprx_calibrate call into guarded buffers: numpy idx [n, K], val, cls, gain, kl [n, 2] (None without)."""
    lib = _ffi.lib()
    n, N = ids.shape
    pi, pv = torch.as_tensor(ids, device="cuda").contiguous(), torch.as_tensor(vals, device="cuda").contiguous()
    tb = table if isinstance(table, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(table, dtype=np.int32), device="cuda")
    bi, bc = (torch.full((n * K + GUARD,), -777, dtype=torch.int32, device="cuda") for _ in range(2))
    bv, bg = (torch.full((n * K + GUARD,), PATTERN, dtype=torch.float32, device="cuda") for _ in range(2))
    bk = torch.full((n * 2 + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    ptr, items = (None, None) if csr is None else csr
    p = lambda x: None if x is None else x.data_ptr()
    rc = lib.bprx_calibrate(e.h, n, N, p(pi), p(pv), row0, p(ptr), p(items), p(tb), int(tb.shape[0]), C, K, float(lam), float(alpha),
                            p(bi), p(bv), p(bc), p(bg), p(bk) if want_kl else None, None)
    _ffi.check(e.h, rc)
    torch.cuda.synchronize()
    for b, fill in ((bi, -777), (bc, -777), (bv, PATTERN), (bg, PATTERN)):
        assert (b[n * K:] == fill).all(), "wrote behind an output"
    assert (bk[2 * n if want_kl else 0:] == PATTERN).all(), "wrote behind kl"
    f = lambda b: b[:n * K].view(n, K).cpu().numpy()
    return f(bi), f(bv), f(bc), f(bg), (bk[:2 * n].view(n, 2).cpu().numpy() if want_kl else None)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b) if x is not None and y is not None)


def _check(tag, ids, vals, table, hists, C, K, lam, alpha, got, sorted_pools=True):
    """The replay described at the top, over all lists of a call, and the exact checks; returns the pool positions."""
    gidx, gval, gcls, ggain, gkl = got
    n, N = ids.shape
    pos = _positions(ids, gidx)                                     # (also: no repeats, -1 past the end)
    M = R.candidates(ids, vals).sum(1)
    T = (pos >= 0).sum(1)
    assert np.array_equal(T, np.minimum(K, M)), "%s: lists of %s picks, candidates %s" % (tag, T.tolist(), M.tolist())
    want_val = np.where(pos >= 0, np.take_along_axis(vals, np.maximum(pos, 0), axis=1), np.float32(0))
    assert np.array_equal(_bits(gval), _bits(want_val.astype(np.float32))), tag
    cc = R.classes_of(ids, table, C)
    assert np.array_equal(gcls, np.where(pos >= 0, np.take_along_axis(cc, np.maximum(pos, 0), axis=1), -1)), tag
    assert (_bits(ggain)[pos < 0] == 0).all() and (_bits(gval)[pos < 0] == 0).all() and (gcls[pos < 0] == -1).all()
    assert (ggain >= 0).all(), tag
    if sorted_pools:                                                # every step of rel and obj is monotone: a class keeps its order
        for r in range(n):
            for c in np.unique(gcls[r, :T[r]]):
                assert (np.diff(pos[r, :T[r]][gcls[r, :T[r]] == c]) > 0).all(), "%s: list %d, class %d out of pool order" % (tag, r, c)
    o64, g64, k64 = R.replay(ids, vals, table, hists, pos, lam, alpha, np.float64, C)
    o32, g32, k32 = R.replay(ids, vals, table, hists, pos, lam, alpha, np.float32, C)
    rows, cols = np.arange(n)[:, None], np.arange(K)[None, :]
    pick64 = o64[rows, cols, np.maximum(pos, 0)]
    with np.errstate(all="ignore"):
        best64 = np.where(pos >= 0, np.nanmax(np.where(np.isnan(o64), -np.inf, o64), axis=2), np.nan)
    gap = float(np.nanmax(best64 - pick64, initial=0.0))
    d_o, a_o = _allowance(o64, o32)
    d_g, a_g = _allowance(g64, g32)
    d_k, a_k = _allowance(k64, k32)
    g_g = float(np.abs(ggain.astype(np.float64) - g64).max())
    g_k = float(np.abs(gkl.astype(np.float64) - k64).max()) if gkl is not None else 0.0
    print("%s: obj float32 deviation %.3e / allowance %.3e / GPU's pick below the float64 best by %.3e" % (tag, d_o, a_o, gap))
    print("%s: gain float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (tag, d_g, a_g, g_g))
    print("%s: kl float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (tag, d_k, a_k, g_k))
    assert not np.isnan(pick64[pos >= 0]).any()
    assert gap <= a_o and g_g <= a_g and g_k <= a_k, tag
    if gkl is not None:
        H = R.history_counts(hists, table, C).sum(1)
        assert (_bits(gkl)[(H == 0) | (T == 0)] == 0).all(), tag
        if lam >= 0.5:
            worse = float((gkl[:, 1].astype(np.float64) - gkl[:, 0]).max())
            print("%s: kl of the calibrated list above the plain list's by %.3e at the most / allowance %.3e" % (tag, worse, a_k))
            assert worse <= a_k, tag
    return pos


# ---- shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_shapes_classes_pools_and_weights(N):
    """Pools of one item, below, at and above a wave and 256 = one slot of every thread; class counts around the workgroup's 256
    threads and at the limit; K = 1, 20 and the whole pool; every lambda and both alphas; the seven kinds of history; 33 lists per
    call and the first of them alone."""
    I, n = 300, 33
    e = _handle()
    for C in CS:
        table = _table(I, C, seed=C)
        hists = _hists(n, I, table, seed=N + C)
        csr = _csr(hists)
        ids, vals = _pools(n, I, N, seed=N + C)
        for K in sorted({1, min(20, N), N}):
            for lam, alpha in MIX:
                tag = "N=%d C=%d K=%d lambda=%g alpha=%g" % (N, C, K, lam, alpha)
                got = _call(e, ids, vals, csr, table, C, K, lam, alpha)
                pos = _check(tag, ids, vals, table, hists, C, K, lam, alpha, got)
                assert _same([g[:1] for g in got], _call(e, ids[:1], vals[:1], csr, table, C, K, lam, alpha)), tag
                if lam == 0.0:
                    assert np.array_equal(got[0], ids[:, :K]) and np.array_equal(_bits(got[1]), _bits(vals[:, :K])), tag
                    assert np.array_equal(_bits(got[4][:, 0]), _bits(got[4][:, 1])), tag
                if K == N:
                    assert (np.sort(pos, axis=1) == np.arange(N)).all(), tag
    e.sync_check()


@pytest.mark.parametrize("n", [1, 33])
def test_the_big_pool_takes_four_slots_per_thread(n):
    """N = 1024: four pool positions per thread.  K = 1 and 20 for every class count; the whole pool (1024 steps) for the first
    three lists at C = 7 and C = 1024."""
    I, N = 1100, 1024
    e = _handle()
    for C in CS:
        table = _table(I, C, seed=C + 1)
        hists = _hists(n, I, table, seed=C)
        csr = _csr(hists)
        ids, vals = _pools(n, I, N, seed=5 + C)
        for K in (1, 20):
            for lam, alpha in MIX:
                tag = "N=1024 n=%d C=%d K=%d lambda=%g alpha=%g" % (n, C, K, lam, alpha)
                got = _call(e, ids, vals, csr, table, C, K, lam, alpha)
                _check(tag, ids, vals, table, hists, C, K, lam, alpha, got)
                if lam == 0.0:
                    assert np.array_equal(got[0], ids[:, :K])
        if C in (7, 1024):
            m = min(n, 3)
            for lam, alpha in ((0.5, 0.01), (1.0, 0.5)):
                got = _call(e, ids[:m], vals[:m], csr, table, C, N, lam, alpha)
                pos = _check("N=K=1024 n=%d C=%d lambda=%g" % (m, C, lam), ids[:m], vals[:m], table, hists[:m], C, N, lam, alpha, got)
                assert (np.sort(pos, axis=1) == np.arange(N)).all()
    e.sync_check()


def test_short_pools_fill_only_their_candidates():
    I, N, C = 300, 70, 7
    e = _handle()
    table = _table(I, C, seed=3)
    for K in (1, 20, 70):
        short = tuple((r, M) for r, M in enumerate((0, 1, 2, K - 1, K, K + 1, 69)) if 0 <= M <= N)
        ids, vals = _pools(8, I, N, seed=9, short=short)
        hists = [np.random.RandomState(r).randint(0, I, 12).tolist() for r in range(8)]
        csr = _csr(hists)
        for lam, alpha in MIX:
            gidx, gval, gcls, ggain, gkl = got = _call(e, ids, vals, csr, table, C, K, lam, alpha)
            _check("short K=%d lambda=%g" % (K, lam), ids, vals, table, hists, C, K, lam, alpha, got)
            for r, M in short:
                T = min(K, M)
                assert (gidx[r, T:] == -1).all() and (_bits(gval[r, T:]) == 0).all() and (gcls[r, T:] == -1).all()
                assert (_bits(ggain[r, T:]) == 0).all() and (gidx[r, :T] >= 0).all() and np.isfinite(gval[r, :T]).all()
                assert T > 0 or (_bits(gkl[r]) == 0).all()
    e.sync_check()


def test_candidates_behind_gaps_are_ranked_by_their_place_among_the_candidates():
    """Slots without a candidate in the MIDDLE of a pool: the plain list of kl[:, 0] is the first T candidates, not the first T slots."""
    I, N, C, K = 300, 70, 7, 10
    e = _handle()
    table = _table(I, C, seed=4)
    ids, vals = _pools(6, I, N, seed=12)
    ids[:, 2:9:2] = -1
    vals[:, 13] = -np.inf
    hists = [np.random.RandomState(40 + r).randint(0, I, 15).tolist() for r in range(6)]
    for lam, alpha in MIX:
        got = _call(e, ids, vals, _csr(hists), table, C, K, lam, alpha)
        _check("gaps lambda=%g" % lam, ids, vals, table, hists, C, K, lam, alpha, got)
        if lam == 0.0:
            keep = [c for c in range(N) if ids[0, c] >= 0 and np.isfinite(vals[0, c])][:K]
            assert got[0][0].tolist() == ids[0, keep].tolist()
    e.sync_check()


def test_two_equal_classes_alternate_at_lambda_one():
    I, N, K = 300, 70, 20
    e = _handle()
    table = (np.arange(I) % 2).astype(np.int32)
    ids, vals = _pools(33, I, N, seed=15)
    assert ((table[ids] == 0).sum(1) >= K).all() and ((table[ids] == 1).sum(1) >= K).all()          # both well stocked
    hists = [[2 * r, 2 * r + 1, 2 * r + 2, 2 * r + 5] for r in range(33)]                               # two of each class
    for alpha in (0.01, 0.5):
        got = _call(e, ids, vals, _csr(hists), table, 2, K, 1.0, alpha)
        _check("two classes alpha=%g" % alpha, ids, vals, table, hists, 2, K, 1.0, alpha, got)
        run = np.cumsum(np.where(got[2] == 0, 1, -1), axis=1)
        assert (np.abs(run) <= 1).all()
    e.sync_check()


# ---- exact: calls, positions, row0, kl == NULL ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,C,lam", [(70, 20, 7, 0.5), (256, 256, 257, 1.0), (65, 1, 2, 0.99), (64, 64, 1024, 0.5), (1024, 20, 255, 0.5)])
def test_a_lists_bits_do_not_depend_on_the_call_its_position_or_row0(N, K, C, lam):
    I = 1100 if N == 1024 else 300
    e = _handle()
    table = _table(I, C, seed=C + 2)
    ids, vals = _pools(33, I, N, seed=N + 1, short=((4, 0), (9, 1), (17, N // 2)))
    hists = _hists(33, I, table, seed=N)
    csr = _csr(hists)
    got = _call(e, ids, vals, csr, table, C, K, lam, 0.01)
    _check("bits N=%d C=%d" % (N, C), ids, vals, table, hists, C, K, lam, 0.01, got)
    assert _same(got, _call(e, ids, vals, csr, table, C, K, lam, 0.01)), "two calls differ"
    perm = np.random.RandomState(N).permutation(33)
    shuf = _call(e, ids[perm], vals[perm], _csr([hists[q] for q in perm]), table, C, K, lam, 0.01)
    assert _same([g[perm] for g in got], shuf), "a list's bits depend on its position"
    for r in (0, 4, 32):                                               # one list, its history found through row0 in the same CSR
        assert _same([g[r:r + 1] for g in got], _call(e, ids[r:r + 1], vals[r:r + 1], csr, table, C, K, lam, 0.01, row0=r)), "row0 = %d" % r
    assert _same(got[:4], _call(e, ids, vals, csr, table, C, K, lam, 0.01, want_kl=False)[:4])           # kl == NULL: the rest unchanged
    bare = _call(e, ids, vals, None, table, C, K, lam, 0.01)                                           # hist_ptr == NULL: every H = 0
    assert np.array_equal(bare[0], _call(e, ids, vals, csr, table, C, K, 0.0, 0.01)[0]) and (_bits(bare[4]) == 0).all()
    assert (_bits(bare[3]) == 0).all()
    e.sync_check()


def test_n_zero_writes_nothing():
    e = _handle()
    lib = _ffi.lib()
    buf = torch.full((GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    bi = torch.full((GUARD,), -777, dtype=torch.int32, device="cuda")
    p = lambda x: x.data_ptr()
    assert lib.bprx_calibrate(e.h, 0, 20, p(bi), p(buf), 0, None, None, p(bi), 5, 3, 5, 0.5, 0.01, p(bi), p(buf), p(bi), p(buf), p(buf),
                              None) == 0
    assert lib.bprx_calibrate(e.h, 0, 20, None, None, 0, None, None, None, 5, 3, 5, 0.5, 0.01, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (buf == PATTERN).all() and (bi == -777).all()
    out = e.calibrate(torch.zeros((0, 20), dtype=torch.int32, device="cuda"), torch.zeros((0, 20), device="cuda"), None,
                      torch.zeros(5, dtype=torch.int32, device="cuda"), 3, 5, 0.5)
    assert [tuple(o.shape) for o in out] == [(0, 5), (0, 5), (0, 5), (0, 5), (0, 2)]
    e.sync_check()


# ---- state ---------------------------------------------------------------------------------------------------------------------
def test_the_call_leaves_the_state_alone():
    """Tables and Adam slots are bit-identical before and after the calls, the calls allocate nothing, and a 6-step run with them
    between steps 3 and 4 ends bit-identical to a run without them (duplicate-free batches)."""
    t = _tables(300, 600, 16, 12, 128, 100, "bf16", seed=17)
    batches = _unique_batches(300, 600, 64, 6, seed=18)
    table_h = _table(600, 7, seed=5)
    hists = _hists(33, 600, table_h, seed=6)
    ids_h, vals_h = _pools(33, 600, 70, seed=19)
    ids, vals = torch.as_tensor(ids_h, device="cuda"), torch.as_tensor(vals_h, device="cuda")
    table, csr = torch.as_tensor(table_h, device="cuda"), _csr(hists)
    lib = _ffi.lib()
    end = []
    for with_calls in (False, True):
        e = _vbpr(t, "bf16", optimizer="adam_tf23", B=64)
        for s, b in enumerate(batches):
            if s == 3 and with_calls:
                e.sync_adam()
                before = _snapshot(e)
                torch.cuda.synchronize()
                held = lib.bprx_live_device_allocs()
                outs = [_call(e, ids_h, vals_h, csr, table, 7, 20, lam, 0.01) for lam in (0.0, 0.5, 1.0)]
                _check("between steps", ids_h, vals_h, table_h, hists, 7, 20, 0.5, 0.01, outs[1])
                out = e.calibrate(ids, vals, csr, table, 7, 20, 0.5)
                torch.cuda.synchronize()
                assert _same(outs[1], [o.cpu().numpy() for o in out])
                del out
                after = _snapshot(e)
                for n in before:
                    assert torch.equal(before[n].view(torch.int32), after[n].view(torch.int32)), n
                # (the guarded buffers of _call and Engine.calibrate's outputs are torch's; the library's own count is unchanged)
                assert lib.bprx_live_device_allocs() == held
            e.step(*b)
        e.sync_check()
        end.append({n: v.cpu().numpy() for n, v in e.t.items() if n != "F"})
        e.close()
    for n in end[0]:
        assert np.array_equal(_bits(end[0][n]), _bits(end[1][n])), "%s: %d words differ" % (
            n, int((_bits(end[0][n]) != _bits(end[1][n])).sum()))


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable_and_no_allocation_behind():
    import test_gpu_acf as ga
    from acf_ref import random_tables
    from fashionvisualexpl_recommend_amd.engine import Engine
    lib = _ffi.lib()
    gc.collect()
    live = lib.bprx_live_device_allocs()
    I, N, K, n, C = 80, 20, 5, 6, 7
    t = _tables(50, I, 16, 12, 256, 200, "bf16", seed=63)
    e = _vbpr(t, "bf16")
    unbound = Engine(model="vbpr", num_users=50, num_items=I, embed_k=16, embed_d=12, feat_dim=256, feat_dtype="bf16", optimizer="sgd",
                     max_batch=64)
    rs = np.random.RandomState(64)
    acf = ga._engine(random_tables(rs, 12, I, 16, 128, 64, 64, scale=10.0), ga._features(rs, I, 9, 128, "fp32"),
                     ga._lists(rs, 12, I, rs.randint(0, 15, 12)))
    table_h = _table(I, C, seed=7)
    hists = _hists(n, I, table_h, seed=8)
    ids_h, vals_h = _pools(n, I, N, seed=65)
    ids, vals, table = (torch.as_tensor(x, device="cuda") for x in (ids_h, vals_h, table_h))
    ptr, items = csr = _csr(hists)
    held = lib.bprx_live_device_allocs()
    good = [x.cpu().numpy() for x in e.calibrate(ids, vals, csr, table, C, K, 0.5)]
    _check("good", ids_h, vals_h, table_h, hists, C, K, 0.5, 0.01, good)
    oi, oc = (torch.full((n * K + GUARD,), -777, dtype=torch.int32, device="cuda") for _ in range(2))
    ov, og, ok = (torch.full((n * K + GUARD,), PATTERN, dtype=torch.float32, device="cuda") for _ in range(3))

    def usable():
        again = [x.cpu().numpy() for x in e.calibrate(ids, vals, csr, table, C, K, 0.5)]
        assert _same(good, again)
        e.sync_check()

    p = lambda x: None if x is None else x.data_ptr()
    call = lambda h, nn=n, NN=N, pi=ids, pv=vals, r0=0, hp=ptr, hi=items, tb=table, w=I, CC=C, KK=K, lam=0.5, al=0.01, a=oi, b=ov, c=oc, \
        g=og, l=ok: lib.bprx_calibrate(h, nn, NN, p(pi), p(pv), r0, p(hp), p(hi), p(tb), w, CC, KK, lam, al, p(a), p(b), p(c), p(g), p(l), None)
    assert call(None) == _ffi.E_INVALID
    nan, inf = float("nan"), float("inf")
    bad = [lambda: call(e.h, pi=None), lambda: call(e.h, pv=None), lambda: call(e.h, tb=None), lambda: call(e.h, hi=None),     # null pointers
           lambda: call(e.h, a=None), lambda: call(e.h, b=None), lambda: call(e.h, c=None), lambda: call(e.h, g=None),
           lambda: call(e.h, nn=-1), lambda: call(e.h, nn=1 << 31), lambda: call(e.h, r0=-1),                                    # ranges
           lambda: call(e.h, KK=0), lambda: call(e.h, KK=-3), lambda: call(e.h, KK=N + 1), lambda: call(e.h, NN=1025, KK=5),
           lambda: call(e.h, NN=0, KK=0), lambda: call(e.h, NN=0, KK=1),
           lambda: call(e.h, CC=0), lambda: call(e.h, CC=-2), lambda: call(e.h, CC=1025), lambda: call(e.h, w=0), lambda: call(e.h, w=-4),
           lambda: call(e.h, lam=-0.01), lambda: call(e.h, lam=1.01), lambda: call(e.h, lam=nan), lambda: call(e.h, lam=inf),
           lambda: call(e.h, al=0.0), lambda: call(e.h, al=1.0), lambda: call(e.h, al=-0.5), lambda: call(e.h, al=1.5),
           lambda: call(e.h, al=nan), lambda: call(e.h, al=inf)]
    for q, c in enumerate(bad):
        assert c() == _ffi.E_INVALID, q
        assert lib.bprx_last_error(e.h).decode().startswith("calibrate"), q
    torch.cuda.synchronize()
    assert (oi == -777).all() and (oc == -777).all() and all((x == PATTERN).all() for x in (ov, og, ok))   # no rejected call wrote
    usable()
    assert call(e.h, l=None) == 0 and call(e.h, lam=0.0) == 0 and call(e.h, lam=1.0) == 0 and call(e.h, hp=None, hi=None) == 0
    assert call(e.h, CC=1024) == 0 and call(e.h, al=0.999) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        e.calibrate(ids.long(), vals, csr, table, C, K, 0.5)             # the pools are int32 / fp32
    with pytest.raises(ValueError):
        e.calibrate(ids, vals, csr, table.long(), C, K, 0.5)             # the class table is int32
    # any handle: unbound tables, an ACF handle -- the bits of the VBPR handle's call
    for eng in (unbound, acf):
        other = [x.cpu().numpy() for x in eng.calibrate(ids, vals, csr, table, C, K, 0.5)]
        assert _same(good, other)
        eng.sync_check()
    assert acf.score_block(0, 12).shape == (12, I)
    usable()
    # a pool id >= width: classless, no fault, reported by sync_check; the returned id is the pool's; the handle stays usable
    wild = ids.clone()
    wild[2, 3] = I + 12345
    out = e.calibrate(wild, vals, csr, table, C, N, 0.5)
    torch.cuda.synchronize()
    assert sorted(out[0][2].tolist()) == sorted(wild[2].tolist())
    assert int(out[2][2][out[0][2] == I + 12345]) == -1
    with pytest.raises(_ffi.BprxError) as err:
        e.sync_check()
    assert err.value.code == _ffi.E_RANGE
    usable()
    # an item_class value outside [-1, C): classless, never an index, reported
    for value in (C, C + 100000, -2, -2 ** 31):
        broken = table.clone()
        broken[int(ids_h[1, 0])] = value
        out = e.calibrate(ids, vals, csr, broken, C, N, 0.5)
        torch.cuda.synchronize()
        assert int(out[2][1][out[0][1] == int(ids_h[1, 0])]) == -1 and sorted(out[0][1].tolist()) == sorted(ids_h[1].tolist())
        with pytest.raises(_ffi.BprxError) as err:
            e.sync_check()
        assert err.value.code == _ffi.E_RANGE, value
        usable()
    assert lib.bprx_live_device_allocs() == held
    for eng in (e, unbound, acf):
        eng.close()
    assert lib.bprx_live_device_allocs() == live


# ---- model ---------------------------------------------------------------------------------------------------------------------
def _calibrated_text(labels, res, H):
    out, ok = io.StringIO(), io.StringIO()
    ranking.write_calibrated(out, ok, labels, *res, H)
    return out.getvalue(), ok.getvalue()


def _model_classes(I=60, C=5, seed=3):
    rs = np.random.RandomState(seed)
    t = rs.randint(0, C, I)
    t[rs.rand(I) < 0.1] = -1
    return t.astype(np.int64)


def test_model_recommend_calibrated():
    table = _model_classes()
    m, raw = _model(calibrate=0.6, calibrate_pool=30, item_classes=table)     # VBPR, bf16, U = 130, I = 60, k = 8, d = 20, top_k = 20
    e, ev = m.engine, m.evaluator
    U, I, K, N, C = 130, 60, 20, 30, 5
    ev.user_block = 48                                                 # three blocks of users
    assert m.calibrate_lambda == 0.6 and m.calibrate_pool == 30 and m.calibrate_alpha == 0.01
    ids, vals, cls, gain, kl = m.recommend_calibrated()
    assert ids.shape == vals.shape == cls.shape == gain.shape == (U, K) and kl.shape == (U, 2) and ids.dtype == cls.dtype == np.int64
    # the pools the lists were picked from: the model's own top-30 (train items masked), as store_recommendation ranks them
    ev._metrics_device_csr()
    pi, pv, _ = ranking.rank_rows(ev._topk(0, U), e.score_block(0, U), N)
    hists = [list(dict.fromkeys(l)) for l in m.data.training_list]
    got = (ids.astype(np.int32), vals, cls.astype(np.int32), gain, kl)
    _check("recommend_calibrated", pi.astype(np.int32), pv, table, hists, C, K, 0.6, 0.01, got)
    for u in range(U):
        assert not set(ids[u].tolist()) & set(m.data.training_list[u])
    assert not np.array_equal(ids, pi[:, :K]) and (kl[:, 1] < kl[:, 0]).any()
    pick = [129, 0, 50, 50, 47, 48]
    assert _same(m.recommend_calibrated(pick), [x[pick] for x in (ids, vals, cls, gain, kl)])
    plain = m.recommend_calibrated(lam=0.0)                              # lambda = 0: the plain lists
    assert np.array_equal(plain[0], pi[:, :K]) and np.array_equal(_bits(plain[1]), _bits(pv[:, :K]))
    other = _model_classes(seed=9)                                     # a table of the caller's
    res = m.recommend_calibrated([3, 4], classes=other, lam=1.0, alpha=0.5)
    _check("classes=", pi[[3, 4]].astype(np.int32), pv[[3, 4]], other, [hists[3], hists[4]], C, K, 1.0, 0.5,
           (res[0].astype(np.int32), res[1], res[2].astype(np.int32), res[3], res[4]))
    assert m.recommend_calibrated([])[0].shape == (0, K)
    assert m.recommend_calibrated([3], k=100, pool=100)[0].shape == (1, I)                         # cut to the catalogue
    for bad in (dict(k=31), dict(pool=1025), dict(lam=1.5), dict(lam=-0.1), dict(alpha=0.0), dict(alpha=1.0), dict(users=[U]),
                dict(classes=np.arange(I) * 40)):                                                 # (more than 1024 classes)
        with pytest.raises(ValueError):
            m.recommend_calibrated(**bad)
    ev.force_host = True
    with pytest.raises(ValueError, match="--calibrate"):
        m.recommend_calibrated()
    ev.force_host = False
    ev.k = 2000
    with pytest.raises(ValueError, match="--calibrate"):
        m.recommend_calibrated()
    e.sync_check()
    e.close()


def test_model_styles_as_classes():
    m, raw = _model(calibrate=0.5, calibrate_pool=30, item_classes="styles", styles=4)
    ids, vals, cls, gain, kl = m.recommend_calibrated()
    assert ids.shape == (130, 20) and (ids >= 0).all() and -1 <= cls.min() and cls.max() < 4
    style = np.full(60, -2, np.int64)
    style[ids.reshape(-1)] = cls.reshape(-1)
    assert np.array_equal(cls, style[ids]) and len(set(style[style >= 0].tolist())) > 1       # one table for the whole call
    assert (kl >= 0).all() and (kl[:, 1] <= kl[:, 0] + 1e-5).all() and (gain >= 0).all()
    m.engine.sync_check()
    m.engine.close()


# ---- files ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", ["vbpr", "bprmf"])
def test_cli_writes_cal_files_next_to_unchanged_recommendations(tmp_path, rec):
    from fashionvisualexpl_recommend_amd import train_rec
    U, Inum, top_k, pool, C = 30, 60, 10, 25, 5
    tr, va, te = synth.make_interactions(U, Inum, per_user=8, seed=53)
    synth.write_dataset(str(tmp_path), "toy", tr, va, te, Inum, features=synth.make_features(Inum, 32, seed=55) if rec == "vbpr" else None)
    rows = [("new shopper", 3), ("b", 7), ("new shopper", 9), ("c 3", 5), ("c 3", 6), ("new shopper", 40), ("c 3", 5)]
    (tmp_path / "new.tsv").write_text("".join("%s\t%d\n" % r for r in rows))
    table = np.random.RandomState(57).randint(0, C, Inum)
    (tmp_path / "classes.tsv").write_text("".join("%d\t%d\n" % (i, c) for i, c in enumerate(table)))
    # --batch_size 1: a step adds at most one term to a gradient row, so runs of the same seed agree bit for bit
    common = ["--rec", rec, "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--reg", "0.01", "--top_k", str(top_k), "--lr", "0.01", "--optimizer", "sgd",
              "--item_classes", str(tmp_path / "classes.tsv")]
    cal = ["--calibrate", "0.5", "--calibrate_pool", str(pool)]
    new = ["--new_users", str(tmp_path / "new.tsv"), "--fold_steps", "9", "--fold_negatives", "3"]
    runs = [[], cal, new, cal + new]
    res = [str(tmp_path / ("res%d" % q)) for q in range(4)]
    for r, extra in zip(res, runs):
        train_rec.train(common + ["--results_root", r] + extra)
    m = train_rec._last_model                                          # (of the last run: it holds the last epoch's tables)
    rdir = [os.path.join(r, "rec_results", "toy", rec) for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] + files[2] if "cal-" in f]
    assert [f for f in files[1] if "cal-" not in f] == files[0] and [f for f in files[3] if "cal-" not in f] == files[2]
    base = [f for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(base) == 2
    read = lambda q, f: open(os.path.join(rdir[q], f), "rb").read()
    for q, p in ((1, 0), (3, 2)):                                      # every other file: the bytes of the run without the flag
        for f in files[p]:
            assert read(q, f) == read(p, f), (f, q)
    for f in base:
        nu = f.replace("recs-", "new-user-recs-", 1)
        names = [os.path.basename(x) for x in ranking.cal_paths(f) + ranking.cal_paths(nu)]
        assert all(x in files[3] for x in names) and all(x in files[1] for x in names[:2]) and not [x for x in names[2:] if x in files[1]]
        assert read(1, names[0]) == read(3, names[0]) and read(1, names[1]) == read(3, names[1])
        got = [l.split("\t") for l in read(3, names[0]).decode().splitlines()]
        plain = [l.split("\t") for l in read(0, f).decode().splitlines()]
        assert len(got) == U * top_k and all(len(r) == 5 for r in got) and [r[0] for r in got] == [r[0] for r in plain]
        for u in range(U):
            blk = got[u * top_k:(u + 1) * top_k]
            assert len({r[1] for r in blk}) == top_k and not {int(r[1]) for r in blk} & set(tr[u])
            assert all(int(r[3]) == table[int(r[1])] and float(r[4]) >= 0.0 for r in blk)
        kl = [l.split("\t") for l in read(3, names[1]).decode().splitlines()]
        assert [r[0] for r in kl] == [str(u) for u in range(U)] and all(len(r) == 4 for r in kl)
        assert all(float(r[1]) >= 0.0 and float(r[2]) >= 0.0 and int(r[3]) == len(set(tr[u])) for u, r in enumerate(kl))
        gn = [l.split("\t") for l in read(3, names[2]).decode().splitlines()]
        assert [r[0] for r in gn] == [lab for lab in ("new shopper", "b", "c 3") for _ in range(top_k)] and all(len(r) == 5 for r in gn)
        kn = [l.split("\t") for l in read(3, names[3]).decode().splitlines()]
        assert [r[0] for r in kn] == ["new shopper", "b", "c 3"] and [int(r[3]) for r in kn] == [3, 1, 2]      # a repeated item once
    # the rows of the last epoch's files are the model's own lists
    last = [f for f in base if f.startswith("recs-")][0]
    once = lambda lists: [list(dict.fromkeys(l)) for l in lists]
    want, want_kl = _calibrated_text(range(U), m.recommend_calibrated(), ranking.hist_classed(once(tr), table))
    p_recs, p_kl = (os.path.basename(x) for x in ranking.cal_paths(last))
    assert read(3, p_recs).decode() == want and read(3, p_kl).decode() == want_kl
    labels, lists = train_rec.read_new_users(str(tmp_path / "new.tsv"))
    want, want_kl = _calibrated_text(labels, m.recommend_new_users(lists, calibrate=0.5, steps=9, negatives=3, seed=0),
                                     ranking.hist_classed(lists, table))
    p_recs, p_kl = (os.path.basename(x) for x in ranking.cal_paths(last.replace("recs-", "new-user-recs-", 1)))
    assert read(3, p_recs).decode() == want and read(3, p_kl).decode() == want_kl
    m.engine.close()


def test_cli_runs_with_the_styles_as_classes(tmp_path):
    from fashionvisualexpl_recommend_amd import train_rec
    U, Inum, top_k = 30, 60, 10
    tr, va, te = synth.make_interactions(U, Inum, per_user=8, seed=53)
    synth.write_dataset(str(tmp_path), "toy", tr, va, te, Inum, features=None)
    train_rec.train(["--rec", "bprmf", "--dataset", "toy", "--data_root", str(tmp_path), "--results_root", str(tmp_path / "res"),
                     "--epochs", "1", "--batch_size", "16", "--embed_k", "16", "--top_k", str(top_k), "--optimizer", "sgd",
                     "--styles", "4", "--item_classes", "styles", "--calibrate", "0.9", "--calibrate_pool", "30"])
    d = os.path.join(str(tmp_path / "res"), "rec_results", "toy", "bprmf")
    names = sorted(os.listdir(d))
    cal = [f for f in names if f.startswith("cal-recs-")]
    st = [f for f in names if f.startswith("styles-")]
    assert len(cal) == 1 and len(st) == 1 and [f for f in names if f.startswith("cal-kl-")]
    style = {int(l.split("\t")[0]): int(l.split("\t")[1]) for l in open(os.path.join(d, st[0]))}
    got = [l.rstrip("\n").split("\t") for l in open(os.path.join(d, cal[0]))]
    assert len(got) == U * top_k and all(int(r[3]) == style[int(r[1])] for r in got)   # one style table per store call
    train_rec._last_model.engine.close()
