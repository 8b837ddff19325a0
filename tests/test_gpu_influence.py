"""bprx_influence on the GPU against the float64 restatement (tests/influence_ref.py).

The kernel (csrc/bprx_influence.hip) walks a row's pairs in tiles of T = 32 and a list in chunks of KC = 8 slots; the rows of a
case have 0, 1, 2, L - 1, L, L + 1, T - 1, T, T + 1 and 2 T + 1 entries, the lists 1, 20, KC - 1, KC and KC + 1 slots with every
seventh slot empty, and per_entry is 1, 4 or 5 with a short last group; one history of every case repeats an id.

Allowance: the project's rule (_allowance of tests/test_gpu_diversify.py): 32 x the max-abs deviation of the float32 restatement
from the float64 one over the case, never below one float32 ulp of the largest magnitude; every comparison prints its triple.
Lists are never compared across precisions: the GPU's picks are replayed against its own out_full with the exact order and tie
rule; out_full, out_infl and out_total are compared with float64 within the allowance.  Every call writes into guarded buffers."""
import gc
import os

import numpy as np
import pytest
import torch

import influence_ref as R
from fashionvisualexpl_recommend_amd import _ffi, synth
from test_gpu_diversify import _allowance
from test_gpu_feat_explain import _bits
from test_gpu_fold_in import _engine, _item_tables
from test_gpu_new_items import GUARD, PATTERN

pytestmark = pytest.mark.gpu

I = 300
T, KC = 32, 8
WIDTHS = [(1, 0), (2, 0), (63, 0), (64, 0), (65, 0), (128, 0), (64, 64), (128, 20), (96, 64), (7, 5)]
DAMPS = [(0.0, 1.0), (0.0, 0.01)]                              # (reg, damp); reg 1e-3 with damp 0 has a test of its own (m >= 4 n)


def _entry_counts(L):
    return [0, 1, 2, L - 1, L, L + 1, T - 1, T, T + 1, 2 * T + 1]


def _rows(counts, pe, seed, short=True):
    """(ptr, pos, neg, ids per row): row r has counts[r] entries of pe pairs (pos = the entry's id); with short, every other row
    with entries loses pairs of its last entry down to one.  Row 4 owns its first id twice."""
    rs = np.random.RandomState(seed)
    pos, neg, ids, ptr = [], [], [], [0]
    for r, E in enumerate(counts):
        h = rs.randint(I, size=E)
        if r == 4 and E > 1:
            h[-1] = h[0]
        m = E * pe - ((pe - 1) if (short and E and r % 2 == 1) else 0)
        pos.append(np.repeat(h, pe)[:m]); neg.append(rs.randint(I, size=m)); ids.append(h)
        ptr.append(ptr[-1] + m)
    return (np.asarray(ptr, np.int64), np.concatenate(pos).astype(np.int32), np.concatenate(neg).astype(np.int32), ids)


def _lists(n, K, seed):
    rs = np.random.RandomState(seed)
    li = rs.randint(I, size=(n, K)).astype(np.int32)
    li.reshape(-1)[6::7] = -1                                   # every seventh slot is empty
    return li


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _call(e, W, ptr, pos, neg, pe, reg, damp, li, L, stride=None, want=("cnt", "full", "flag")):
    """One bprx_influence call into guarded buffers: dict of numpy outputs (full [n, K, stride] with PATTERN where unwritten)."""
    n, K = li.shape
    k, d = e.k, e.d
    stride = max(1, int(-(-(np.diff(ptr).max(initial=0)) // pe))) if stride is None else stride
    Gu, Tu = _dev(W[:, :k]), (_dev(W[:, k:]) if d else None)
    bi = torch.full((n * K * L + GUARD,), -777, dtype=torch.int32, device="cuda")
    bv = torch.full((n * K * L + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    bt = torch.full((n * K + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    bc = torch.full((n * K + GUARD,), -777, dtype=torch.int32, device="cuda")
    bf = torch.full((n * K * stride + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    bg = torch.full((n + GUARD,), -777, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    dptr, dpos, dneg, dli = (_dev(x) for x in (ptr, pos, neg, li))     # (held until the call has run: a temporary's memory is reused)
    rc = e.lib.bprx_influence(e.h, p(Gu), p(Tu), n, p(dptr), p(dpos), p(dneg), pe, reg, damp, K, p(dli), L,
                              p(bi), p(bv), p(bt), p(bc) if "cnt" in want else None, p(bf) if "full" in want else None, stride,
                              p(bg) if "flag" in want else None, None)
    _ffi.check(e.h, rc)
    torch.cuda.synchronize()
    assert (bi[n * K * L:] == -777).all() and (bv[n * K * L:] == PATTERN).all() and (bt[n * K:] == PATTERN).all(), "wrote behind an output"
    assert (bc[n * K if "cnt" in want else 0:] == -777).all() and (bg[n if "flag" in want else 0:] == -777).all(), "wrote behind cnt / flag"
    assert (bf[n * K * stride if "full" in want else 0:] == PATTERN).all(), "wrote behind full"
    out = {"item": bi[:n * K * L].view(n, K, L).cpu().numpy(), "infl": bv[:n * K * L].view(n, K, L).cpu().numpy(),
           "total": bt[:n * K].view(n, K).cpu().numpy()}
    if "cnt" in want:
        out["cnt"] = bc[:n * K].view(n, K).cpu().numpy()
    if "full" in want:
        out["full"] = bf[:n * K * stride].view(n, K, stride).cpu().numpy()
    if "flag" in want:
        out["flag"] = bg[:n].cpu().numpy()
    return out


def _P(e):
    """The item projections the handle holds, [I, d + 1] (current after any call that reads them)."""
    return e.item_proj().cpu().numpy()[:, :e.d + 1] if e.d else None


def _refs(e, t, W, ptr, pos, neg, pe, reg, damp, li):
    k, d = e.k, e.d
    P = _P(e)
    return tuple(R.influence(t["Gi"], t["Bi"], P, W[:, :k], W[:, k:] if d else None, ptr, pos, neg, pe, reg, damp, li, dt)
                 for dt in (np.float64, np.float32))


def _pattern():
    return np.float32(PATTERN)


def _check(tag, out, r64, r32, ptr, pos, pe, li, L):
    """Counts, flags and the written extent exactly; out_full and out_total against float64 within the allowance; the lists
    replayed against the GPU's own out_full."""
    n, K = li.shape
    assert np.array_equal(out["flag"], r64["flag"]) and np.array_equal(out["cnt"], r64["cnt"]), tag
    assert not np.isnan(out["infl"]).any() and not np.isnan(out["total"]).any()
    f64 = np.concatenate([f[~np.isnan(f)].reshape(-1) for f in r64["full"]] + [np.zeros(1)])
    f32 = np.concatenate([f[~np.isnan(f)].reshape(-1) for f in r32["full"]] + [np.zeros(1, np.float32)])
    dev, allow = _allowance(f64, f32)
    tdev, tallow = _allowance(r64["total"], r32["total"])
    gdev = gt = 0.0
    for r in range(n):
        m = int(ptr[r + 1] - ptr[r])
        M = -(-m // pe)
        ids = pos[ptr[r]:ptr[r + 1]][::pe]
        for q in range(K):
            full = out["full"][r, q]
            on = li[r, q] >= 0 and M > 0 and not r64["flag"][r]
            assert (_bits(full[M if on else 0:]) == _bits(_pattern())).all(), "%s: (%d, %d) wrote past its entries" % (tag, r, q)
            if not on:
                assert (out["item"][r, q] == -1).all() and not out["infl"][r, q].any() and out["total"][r, q] == 0 and out["cnt"][r, q] == 0
                continue
            got = full[:M]
            gdev = max(gdev, float(np.abs(got.astype(np.float64) - r64["full"][r][q]).max()))
            gt = max(gt, abs(float(out["total"][r, q]) - float(r64["total"][r, q])))
            order = R.top_entries(got, L)                        # the GPU's own values, the exact rule
            kk = len(order)
            assert np.array_equal(out["item"][r, q, :kk], ids[order]), "%s: (%d, %d) picks" % (tag, r, q)
            assert np.array_equal(_bits(out["infl"][r, q, :kk]), _bits(got[order])), "%s: (%d, %d) values" % (tag, r, q)
            assert (out["item"][r, q, kk:] == -1).all() and not out["infl"][r, q, kk:].any()
    print("%s: full float32 deviation %.3e / allowance %.3e / GPU deviation %.3e; total %.3e / %.3e / %.3e"
          % (tag, dev, allow, gdev, tdev, tallow, gt))
    assert gdev <= allow, "%s: out_full %.3e > %.3e" % (tag, gdev, allow)
    assert gt <= tallow, "%s: out_total %.3e > %.3e" % (tag, gt, tallow)


def _W(n, w, seed):
    return (np.random.RandomState(seed).standard_normal((n, w)) * 0.3).astype(np.float32)


_engines = {}


def _eng(k, d):
    if (k, d) not in _engines:
        t = _item_tables(k, d, seed=k + d)
        _engines[(k, d)] = (t, _engine(t))
    return _engines[(k, d)]


# ---- shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(WIDTHS)))
def test_widths_entry_counts_and_lists_against_float64(case):
    """Every width on a BPRMF (d = 0) or VBPR handle; per_entry, K, L and the damping cycle with the case."""
    k, d = WIDTHS[case]
    t, e = _eng(k, d)
    pe = (1, 4, 5)[case % 3]
    K = (1, 20, KC - 1, KC, KC + 1)[case % 5]
    L = (1, 5, 32)[(case // 2) % 3]
    reg, damp = DAMPS[case % 2]
    counts = _entry_counts(L)
    ptr, pos, neg, _ = _rows(counts, pe, seed=100 + case)
    W, li = _W(len(counts), k + d, 200 + case), _lists(len(counts), K, 300 + case)
    out = _call(e, W, ptr, pos, neg, pe, reg, damp, li, L)
    r64, r32 = _refs(e, t, W, ptr, pos, neg, pe, reg, damp, li)
    _check("k %d d %d pe %d K %d L %d damp %g" % (k, d, pe, K, L, damp), out, r64, r32, ptr, pos, pe, li, L)
    e.sync_check()


@pytest.mark.parametrize("pe,K,L", [(1, KC + 1, 32), (4, 20, 5), (5, KC - 1, 1), (4, KC, 32), (5, 1, 5)])
def test_per_entry_list_lengths_and_tops_at_the_benchmark_width(pe, K, L):
    k, d = 64, 64
    t, e = _eng(k, d)
    counts = _entry_counts(L)
    ptr, pos, neg, _ = _rows(counts, pe, seed=400 + pe + K)
    W, li = _W(len(counts), k + d, 401), _lists(len(counts), K, 402 + K)
    for reg, damp in DAMPS:
        out = _call(e, W, ptr, pos, neg, pe, reg, damp, li, L)
        r64, r32 = _refs(e, t, W, ptr, pos, neg, pe, reg, damp, li)
        _check("pe %d K %d L %d damp %g" % (pe, K, L, damp), out, r64, r32, ptr, pos, pe, li, L)
    e.sync_check()


@pytest.mark.parametrize("k,d", [(7, 5), (16, 0)])
def test_the_plain_ridge_without_damping(k, d):
    """damp = 0 with reg = 1e-3: rows with m >= 4 n pairs, where A alone is well conditioned."""
    t, e = _eng(k, d)
    n, pe, K, L = k + d, 4, 20, 5
    counts = [n, n + 1, 2 * n + 3, -(-(4 * n) // pe) + 7]
    ptr, pos, neg, _ = _rows(counts, pe, seed=500 + k, short=False)
    assert (np.diff(ptr) >= 4 * n).all()
    W, li = _W(len(counts), n, 501), _lists(len(counts), K, 502)
    out = _call(e, W, ptr, pos, neg, pe, 1e-3, 0.0, li, L)
    r64, r32 = _refs(e, t, W, ptr, pos, neg, pe, 1e-3, 0.0, li)
    _check("ridge k %d d %d" % (k, d), out, r64, r32, ptr, pos, pe, li, L)
    e.sync_check()


# ---- independence --------------------------------------------------------------------------------------------------------------
def test_a_rows_bits_depend_on_nothing_but_the_row():
    """The same rows at other positions, in a call with another n and K: the same bits; NULL cnt / full / flag change nothing."""
    k, d = 64, 64
    t, e = _eng(k, d)
    pe, K, L = 4, 20, 5
    counts = _entry_counts(L)
    ptr, pos, neg, _ = _rows(counts, pe, seed=600)
    n = len(counts)
    W, li = _W(n, k + d, 601), _lists(n, K, 602)
    stride = int(-(-np.diff(ptr).max() // pe))
    a = _call(e, W, ptr, pos, neg, pe, 0.0, 1.0, li, L, stride=stride)
    b = _call(e, W, ptr, pos, neg, pe, 0.0, 1.0, li, L, stride=stride, want=())
    for name in ("item", "infl", "total"):
        assert np.array_equal(_bits(a[name]), _bits(b[name])), name
    pick = [9, 3, 7, 2]                                          # other positions, another n; the first 11 slots: another K, other chunks
    cnt = [int(ptr[r + 1] - ptr[r]) for r in pick]
    ptr2 = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in pick]).astype(np.int64)
    K2 = 11
    c = _call(e, W[pick], ptr2, pos[take], neg[take], pe, 0.0, 1.0, np.ascontiguousarray(li[pick][:, :K2]), L, stride=stride)
    for name in ("item", "infl", "total", "cnt", "full"):
        assert np.array_equal(_bits(a[name][pick][:, :K2]), _bits(c[name])), name
    assert np.array_equal(a["flag"][pick], c["flag"])
    e.sync_check()


# ---- flag ----------------------------------------------------------------------------------------------------------------------
def test_a_failed_factorisation_flags_the_row_and_leaves_its_neighbours_alone():
    """Rows whose pairs name items with all-zero rows (A = 0, reg = 0): flag 1, empty slots, no NaN; the other rows as alone."""
    k, d = 16, 12
    t = _item_tables(k, d, seed=77)
    t["Gi"][:20] = 0
    t["F"][:20] = 0
    e = _engine(t)
    pe, K, L = 4, 9, 5
    counts = [5, 6, 0, 7, 33]
    ptr, pos, neg, _ = _rows(counts, pe, seed=700, short=False)
    rs = np.random.RandomState(701)
    for r in (1, 3):                                             # every item of these rows is a zero row
        pos[ptr[r]:ptr[r + 1]] = rs.randint(20, size=ptr[r + 1] - ptr[r])
        neg[ptr[r]:ptr[r + 1]] = rs.randint(20, size=ptr[r + 1] - ptr[r])
    W, li = _W(len(counts), k + d, 702), _lists(len(counts), K, 703)
    out = _call(e, W, ptr, pos, neg, pe, 0.0, 1.0, li, L)
    assert out["flag"].tolist() == [0, 1, 0, 1, 0]
    r64, r32 = _refs(e, t, W, ptr, pos, neg, pe, 0.0, 1.0, li)
    assert r64["flag"].tolist() == [0, 1, 0, 1, 0]
    _check("flag", out, r64, r32, ptr, pos, pe, li, L)
    keep = [0, 4]
    cnt = [int(ptr[r + 1] - ptr[r]) for r in keep]
    take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in keep]).astype(np.int64)
    alone = _call(e, W[keep], np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), pos[take], neg[take], pe, 0.0, 1.0,
                  np.ascontiguousarray(li[keep]), L, stride=out["full"].shape[2])
    for name in ("item", "infl", "total", "cnt", "full", "flag"):
        assert np.array_equal(_bits(out[name][keep]), _bits(alone[name])), name
    e.sync_check()
    e.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------
def test_the_call_reads_current_tables_after_lazy_adam_steps_with_a_pending_dense_update(monkeypatch):
    """After three bprx_step calls (lazy adam_tf23, the dense update deferred): the call equals float64 computed from the tables
    read through Engine.t."""
    from test_gpu_feat_explain import _tables, _unique_batches, _vbpr
    monkeypatch.setenv("BPRX_ADAM_LAZY", "1")
    t0 = _tables(300, I, 16, 12, 128, 100, "bf16", seed=17)
    e = _vbpr(t0, "bf16", optimizer="adam_tf23", B=64)
    assert e.adam_is_lazy()
    for b in _unique_batches(300, I, 64, 3, seed=18):
        e.step(*b, want_loss=False)
    pe, K, L = 4, 9, 5
    counts = [3, 0, 9, 40]
    ptr, pos, neg, _ = _rows(counts, pe, seed=800)
    users = [5, 17, 100, 250]
    li = _lists(len(counts), K, 801)
    Gu, Tu = e.t["Gu"], e.t["Tu"]                               # (the handle's own rows of trained users, gathered after the call below settles them)
    W0 = np.zeros((len(users), 28), np.float32)
    _call(e, W0, ptr, pos, neg, pe, 0.0, 1.0, li, L)             # brings rows, E | Bp and P up to date: what any reader goes through
    assert not e.dense_pending()
    t = {n: v.cpu().numpy() for n, v in e.t.items() if n != "F"}
    W = np.concatenate([t["Gu"][users], t["Tu"][users]], 1)
    out = _call(e, W, ptr, pos, neg, pe, 0.0, 1.0, li, L)
    r64, r32 = _refs(e, t, W, ptr, pos, neg, pe, 0.0, 1.0, li)
    _check("after steps", out, r64, r32, ptr, pos, pe, li, L)
    # a fresh handle run the same way, asked once: the first call after the steps gives the same bits
    e2 = _vbpr(t0, "bf16", optimizer="adam_tf23", B=64)
    for b in _unique_batches(300, I, 64, 3, seed=18):
        e2.step(*b, want_loss=False)
    first = _call(e2, W, ptr, pos, neg, pe, 0.0, 1.0, li, L)
    for name in ("item", "infl", "total", "cnt", "full", "flag"):
        assert np.array_equal(_bits(out[name]), _bits(first[name])), name
    for eng in (e, e2):
        eng.sync_check()
        eng.close()


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable_and_no_allocation_behind():
    import test_gpu_acf as ga
    from acf_ref import random_tables
    from fashionvisualexpl_recommend_amd.engine import Engine
    lib = _ffi.lib()
    gc.collect()
    live = lib.bprx_live_device_allocs()
    t = _item_tables(16, 12, seed=70)
    e = _engine(t)
    wide = Engine(model="bprmf", num_users=2, num_items=4, embed_k=161, optimizer="sgd", max_batch=8)
    wide.bind(np.zeros((2, 161), np.float32), np.zeros((4, 161), np.float32), np.zeros(4, np.float32))
    unbound = Engine(model="bprmf", num_users=8, num_items=I, embed_k=16, optimizer="sgd", max_batch=8)
    rs = np.random.RandomState(71)
    acf = ga._engine(random_tables(rs, 6, 20, 16, 8, 4, 4), ga._features(rs, 20, 2, 8, "fp32"), ga._lists(rs, 6, 20, [2, 0, 3, 1, 2, 2]))
    n, K, L, pe = 2, 3, 2, 2
    ptr, pos, neg = _dev(np.array([0, 4, 6], np.int64)), _dev(np.array([1, 1, 2, 2, 3, 3], np.int32)), _dev(np.array([4, 5, 6, 7, 8, 9], np.int32))
    li = _dev(np.array([[1, 2, -1], [3, 4, 5]], np.int32))
    Gu, Tu = _dev(_W(2, 16, 72)), _dev(_W(2, 12, 73))
    oi = torch.full((n * K * L + GUARD,), -777, dtype=torch.int32, device="cuda")
    ov = torch.full((n * K * L + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    ot = torch.full((n * K + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    oc = torch.full((n * K + GUARD,), -777, dtype=torch.int32, device="cuda")
    of = torch.full((n * K * 2 + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    og = torch.full((n + GUARD,), -777, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    held = lib.bprx_live_device_allocs()
    p = lambda x: None if x is None else x.data_ptr()

    def call(h, G=Gu, Tt=Tu, nn=n, pp=ptr, a=pos, b=neg, per=pe, reg=0.0, damp=1.0, KK=K, l=li, LL=L, i=oi, v=ov, tt=ot, c=oc, f=of,
             st=2, g=og):
        return lib.bprx_influence(h, p(G), p(Tt), nn, p(pp), p(a), p(b), per, reg, damp, KK, p(l), LL, p(i), p(v), p(tt), p(c), p(f),
                                  st, p(g), None)

    assert call(e.h) == 0
    torch.cuda.synchronize()
    good = [x.clone() for x in (oi, ov, ot, oc, of, og)]
    assert (oi[n * K * L:] == -777).all() and (of[n * K * 2:] == PATTERN).all() and og[:n].tolist() == [0, 0]
    for x, fill in ((oi, -777), (ov, PATTERN), (ot, PATTERN), (oc, -777), (of, PATTERN), (og, -777)):
        x.fill_(fill)
    assert call(None) == _ffi.E_INVALID
    assert call(e.h, nn=0) == 0 and call(e.h, nn=0, a=None, b=None, l=None, i=None, v=None, tt=None) == 0
    inf, nan = float("inf"), float("nan")
    for kw in (dict(nn=-1), dict(nn=1 << 31), dict(KK=0), dict(KK=1025), dict(LL=0), dict(LL=33), dict(per=0), dict(reg=-1.0),
               dict(damp=-1.0), dict(reg=inf), dict(damp=inf), dict(reg=nan), dict(damp=nan), dict(reg=0.0, damp=0.0), dict(st=0),
               dict(G=None), dict(Tt=None), dict(pp=None), dict(a=None), dict(b=None), dict(l=None), dict(i=None), dict(v=None),
               dict(tt=None)):
        assert call(e.h, **kw) == _ffi.E_INVALID, kw
    assert call(acf.h, Tt=None) == _ffi.E_INVALID
    G161 = torch.zeros((2, 161), device="cuda")
    assert call(wide.h, G=G161, Tt=None) == _ffi.E_INVALID and "160" in lib.bprx_last_error(wide.h).decode()
    assert call(unbound.h, Tt=None) == _ffi.E_STATE
    torch.cuda.synchronize()
    assert (oi == -777).all() and (ov == PATTERN).all() and (ot == PATTERN).all() and (oc == -777).all() and (of == PATTERN).all() \
        and (og == -777).all()                                   # no rejected call wrote anything
    assert call(e.h, st=0, f=None) == 0 and call(e.h, c=None, g=None) == 0 and call(e.h) == 0
    torch.cuda.synchronize()
    for x, y in zip((oi, ov, ot, oc, of, og), good):             # usable: the bits of the first call
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    e.sync_check()
    bad = _dev(np.array([1, 1, I, 2, 3, 3], np.int32))
    assert call(e.h, a=bad) == 0                                 # an id out of range: clamped and reported, once
    with pytest.raises(_ffi.BprxError) as err:
        e.sync_check()
    assert err.value.code == _ffi.E_RANGE
    assert call(e.h) == 0
    e.sync_check()
    assert lib.bprx_live_device_allocs() == held                 # the calls allocated nothing
    for eng in (e, wide, unbound, acf):
        eng.close()
    assert lib.bprx_live_device_allocs() == live


# ---- model methods -------------------------------------------------------------------------------------------------------------
def _model(rec):
    from argparse import Namespace
    from fashionvisualexpl_recommend_amd.models import GradFashion
    from test_gpu_fold_in import _model as fold_model
    if rec != "grad_fashion":
        return fold_model(rec, fold_negatives=3)
    from test_gpu_gradfashion import _data, _params
    U, Inum = 130, 60
    rs = np.random.RandomState(47)
    p = _params(optimizer="sgd", fold_negatives=3)
    data = _data(U, Inum, p)
    return GradFashion(data, p, features=(rs.rand(Inum, 10) * 9.0, synth.make_features(Inum, 21, seed=48))), data.training_list


def _model_refs(m, Gu, Tu, ptr, pos, neg, pe, reg, damp, li):
    eng = m.engine
    t = {n: eng.t[n].cpu().numpy() for n in ("Gi", "Bi")}
    P = _P(eng)
    return tuple(R.influence(t["Gi"], t["Bi"], P, Gu, Tu, ptr, pos, neg, pe, reg, damp, li, dt) for dt in (np.float64, np.float32))


@pytest.mark.parametrize("rec", ["bprmf", "vbpr", "grad_fashion"])
def test_model_influence_for_pairs_in_any_order_and_for_folded_users(rec):
    """models.influence on a BPRMF, a VBPR and a factored (GradFashion) handle: pairs in arbitrary order against float64 from the
    tables the engine holds, maps=True returns the full map, and rows= / lists= serve folded-in users with the pairs that fitted
    them."""
    from fashionvisualexpl_recommend_amd.models import draw_fold_pairs
    m, tr = _model(rec)
    eng, Inum = m.engine, m.num_items
    users = np.array([7, 7, 3, 3, 3, 7, 50, 129, 129], np.int64)
    items = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9], np.int64)
    hist, infl, total, cnt, full = m.influence(users, items, top=4, maps=True)
    assert hist.shape == infl.shape == (9, 4) and total.shape == cnt.shape == (9,) and full.shape[0] == 9
    runs = [7, 3, 7, 50, 129]                                    # the call's lists: one draw over their histories, in order
    ptr, pos, neg = draw_fold_pairs([tr[u] for u in runs], Inum, 3, 5)
    li = np.array([[1, 2, -1], [3, 4, 5], [6, -1, -1], [7, -1, -1], [8, 9, -1]])
    Gu = eng.t["Gu"].cpu().numpy()[runs]
    Tu = eng.t["Tu"].cpu().numpy()[runs] if eng.d else None
    r64, r32 = _model_refs(m, Gu, Tu, ptr, pos, neg, 3, m.reg, 1.0, li)
    slot = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 0), (3, 0), (4, 0), (4, 1)]
    f64 = np.concatenate([r64["full"][r][q] for r, q in slot])
    f32 = np.concatenate([r32["full"][r][q] for r, q in slot])
    dev, allow = _allowance(f64, f32)
    gdev = 0.0
    for p, (r, q) in enumerate(slot):
        M = r64["full"][r].shape[1]
        assert cnt[p] == M == len(tr[runs[r]]) and not full[p, M:].any()
        gdev = max(gdev, float(np.abs(full[p, :M] - r64["full"][r][q]).max()))
        order = R.top_entries(full[p, :M], 4)
        assert np.array_equal(hist[p, :len(order)], np.asarray(tr[runs[r]])[order]) and (hist[p, len(order):] == -1).all()
        assert np.array_equal(_bits(infl[p, :len(order)]), _bits(full[p, :M][order]))
        assert abs(float(total[p]) - float(r64["total"][r, q])) <= _allowance(r64["total"], r32["total"])[1]
    print("model %s: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (rec, dev, allow, gdev))
    assert gdev <= allow
    again = m.influence(users, items, top=4)                     # without maps: the same lists
    assert len(again) == 4 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, (hist, infl, total, cnt)))
    # folded-in users: the fitted rows, the lists that fitted them, the same negatives and seed
    new = [list(tr[4]), [], list(tr[9]) + list(tr[9][:2])]
    fold = dict(steps=6, negatives=3, seed=5)
    Gn, Tn = m.fold_in_users(new, **fold)
    nu, ni = np.repeat(np.arange(3), 5), np.tile(np.array([2, 11, 23, 40, 59]), 3)
    h2, i2, t2, c2, f2 = m.influence(nu, ni, top=3, rows=(Gn, Tn), lists=new, maps=True)
    ptr, pos, neg = draw_fold_pairs(new, Inum, 3, 5)
    r64, r32 = _model_refs(m, Gn.cpu().numpy(), Tn.cpu().numpy() if eng.d else None, ptr, pos, neg, 3, m.reg, 1.0, ni.reshape(3, 5))
    dev, allow = _allowance(np.concatenate([f.reshape(-1) for f in r64["full"]]), np.concatenate([f.reshape(-1) for f in r32["full"]]))
    assert c2.reshape(3, 5).tolist() == [[len(new[0])] * 5, [0] * 5, [len(new[2])] * 5] and (h2[5:10] == -1).all() and not t2[5:10].any()
    gdev = max(float(np.abs(f2.reshape(3, 5, -1)[r][:, :len(new[r])] - r64["full"][r]).max()) for r in (0, 2))
    print("model %s, folded users: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (rec, dev, allow, gdev))
    assert gdev <= allow
    with pytest.raises(ValueError):
        m.influence([0], [1], top=33)
    with pytest.raises(ValueError):
        m.influence([m.num_users], [1])
    eng.sync_check()
    eng.close()


# ---- files ---------------------------------------------------------------------------------------------------------------------
def test_cli_writes_influence_files_next_to_unchanged_recommendations(tmp_path):
    from fashionvisualexpl_recommend_amd import train_rec
    U, Inum, top_k = 30, 60, 5
    tr, va, te = synth.make_interactions(U, Inum, per_user=8, seed=53)
    synth.write_dataset(str(tmp_path), "toy", tr, va, te, Inum, features=synth.make_features(Inum, 32, seed=55))
    rows = [("new shopper", 3), ("b", 7), ("new shopper", 9), ("c 3", 5), ("c 3", 6), ("new shopper", 40), ("c 3", 5)]
    (tmp_path / "new.tsv").write_text("".join("%s\t%d\n" % r for r in rows))
    # --batch_size 1: a step adds at most one term to a gradient row, so runs of the same seed agree bit for bit
    common = ["--rec", "vbpr", "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--reg", "0.01", "--top_k", str(top_k), "--lr", "0.01", "--optimizer", "sgd",
              "--new_users", str(tmp_path / "new.tsv"), "--fold_steps", "9", "--fold_negatives", "3"]
    res = [str(tmp_path / ("res%d" % q)) for q in range(2)]
    train_rec.train(common + ["--results_root", res[0]])
    train_rec.train(common + ["--results_root", res[1], "--influence", "3"])
    rdir = [os.path.join(r, "rec_results", "toy", "vbpr") for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    added = sorted(set(files[1]) - set(files[0]))
    assert not [f for f in files[0] if "influence" in f] and set(files[0]) <= set(files[1])
    assert len(added) == 4 and sorted(f.split("-recs")[0].rstrip("-0123456789") for f in added if "new-user" in f) == \
        ["best-influence-new-user", "influence-new-user"]
    for f in files[0]:                                               # every other file: the bytes of the run without the flag
        assert open(os.path.join(rdir[0], f), "rb").read() == open(os.path.join(rdir[1], f), "rb").read(), f
    for base in [f for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]:
        for kind, src in (("influence", base), ("influence-new-user-recs", base.replace("recs-", "new-user-recs-", 1))):
            name = base.replace("recs-", kind + "-", 1)
            assert name in added, name
            want = [l.rstrip("\n") for l in open(os.path.join(rdir[1], src))]
            got = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], name))]
            assert all(len(r) == 7 for r in got)
            heads = list(dict.fromkeys("\t".join(r[:3]) for r in got))
            assert heads == want                                     # every pair of the list file is named, in order
            for h in heads:
                blk = [r for r in got if "\t".join(r[:3]) == h]
                assert [int(r[3]) for r in blk] == list(range(len(blk))) and 1 <= len(blk) <= 3       # (every user here has entries)
                v = [float(r[5]) for r in blk]
                assert v == sorted(v, reverse=True) and all(0 <= int(r[4]) < Inum for r in blk)
                assert sum(abs(float(r[6])) for r in blk) <= 1.0 + 1e-5
                for r in blk:                                        # share = influence / total, one total per pair
                    assert (float(r[6]) >= 0) == (float(r[5]) >= 0) or float(r[6]) == 0
