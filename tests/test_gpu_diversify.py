"""Diversified lists on the MI355X: bprx_diversify against the float64 restatement (tests/diversify_ref.py), the model methods on
top of it and the div-* files of train_rec --diversify.

A greedy choice is discontinuous, so list identities are never compared across precisions and no near-tie is left out: the GPU's
OWN list is replayed in float64.  At each step, given the GPU's prefix, the float64 objective of the GPU's pick must lie within
the allowance of the largest float64 objective among the remaining candidates, and the GPU's penalty within the allowance of the
float64 one; the same for ild; val is bit-equal to the pool's score at the returned id.

Allowance per compared output (the rule of tests/test_gpu_feat_explain.py): 32 x the max-abs deviation of the FLOAT32 restatement
(replaying the same list) from the float64 one over the case, never below one float32 ulp of the output's largest magnitude.
Every comparison prints its triple (float32 deviation / allowance / GPU deviation).  What is exact is checked exactly."""
import gc
import io
import os

import numpy as np
import pytest
import torch

import diversify_ref as R
import similar_ref as S
from fashionvisualexpl_recommend_amd import _ffi, ranking, synth
from test_gpu_feat_explain import _bits, _snapshot, _tables, _unique_batches, _vbpr
from test_gpu_new_items import GUARD, PATTERN, _model
from test_gpu_similar import FEAT_D, _bprmf

pytestmark = pytest.mark.gpu

_REF = {}
NS = (1, 20, 63, 64, 65, 70, 256)
THETAS = (0.0, 0.3, 1.0)


def _case(I, k, d, dtype, special=False):
    """Tables and, per space, (z64, z32): the item vectors in float64 and float32.  Computed once per case and left unchanged.
    special: items 7 and 19 are twins (bit-equal Gi, F, Bi)."""
    key = (I, k, d, dtype, special)
    if key not in _REF:
        t = _tables(40, I, k, d, FEAT_D[dtype], 390, dtype, seed=70 + k + d)
        if special:
            t["Gi"][19], t["F"][19], t["Bi"][19] = t["Gi"][7], t["F"][7], t["Bi"][7]
        z = {sp: tuple(S.item_vectors(t, sp, dtype, dt) for dt in (torch.float64, torch.float32)) for sp in S.SPACES}
        _REF[key] = (t, z)
    return _REF[key]


def _pools(n, I, N, seed, short=()):
    """n pools of N of I items as the top-K entries return them: distinct ids by descending score.  short: (row, M) pairs, row keeps
    M candidates and ends in -1 / 0.0 slots and then in masked items with -inf (a user with fewer than N unmasked items)."""
    rs = np.random.RandomState(seed)
    sc = rs.standard_normal((n, I)).astype(np.float32) * 3
    ids = np.argsort(-sc, axis=1, kind="stable")[:, :N].astype(np.int32)
    vals = np.take_along_axis(sc, ids.astype(np.int64), axis=1)
    for r, M in short:
        cut = M + (N - M) // 2
        ids[r, M:cut], vals[r, M:cut] = -1, 0.0
        vals[r, cut:] = -np.inf
    return ids, vals


def _call(e, space, rn, ids, vals, K, theta, want_ild=True):
    """One bprx_diversify call into guarded buffers: numpy idx [n, K], val, pen, ild [n] (None without)."""
    lib = _ffi.lib()
    n, N = ids.shape
    pi, pv = torch.as_tensor(ids, device="cuda").contiguous(), torch.as_tensor(vals, device="cuda").contiguous()
    bi = torch.full((n * K + GUARD,), -777, dtype=torch.int32, device="cuda")
    bv, bp = (torch.full((n * K + GUARD,), PATTERN, dtype=torch.float32, device="cuda") for _ in range(2))
    bl = torch.full((n + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    rc = lib.bprx_diversify(e.h, _ffi.SIM_SPACE[space], rn.data_ptr(), n, N, pi.data_ptr(), pv.data_ptr(), K, float(theta),
                            bi.data_ptr(), bv.data_ptr(), bp.data_ptr(), bl.data_ptr() if want_ild else None, None)
    _ffi.check(e.h, rc)
    torch.cuda.synchronize()
    assert (bi[n * K:] == -777).all() and (bv[n * K:] == PATTERN).all() and (bp[n * K:] == PATTERN).all(), "wrote behind an output"
    assert (bl[n if want_ild else 0:] == PATTERN).all(), "wrote behind ild"
    f = lambda b: b[:n * K].view(n, K).cpu().numpy()
    return f(bi), f(bv), f(bp), (bl[:n].cpu().numpy() if want_ild else None)


def _positions(ids, gidx):
    """Pool positions [n, K] of the returned ids (-1 stays -1); a returned id is a candidate of its pool, once."""
    pos = np.full(gidx.shape, -1, np.int64)
    for r in range(gidx.shape[0]):
        where = {int(i): c for c, i in enumerate(ids[r]) if i >= 0}
        got = [int(i) for i in gidx[r] if i >= 0]
        assert len(set(got)) == len(got), "list %d repeats an item" % r
        pos[r, :len(got)] = [where[i] for i in got]
        assert (gidx[r, len(got):] == -1).all()
    return pos


def _allowance(a64, a32):
    dev = float(np.nanmax(np.abs(a64 - a32.astype(np.float64)), initial=0.0))
    return dev, max(32.0 * dev, float(np.spacing(np.float32(np.nanmax(np.abs(a64), initial=0.0)))))


def _check(tag, ids, vals, z64, z32, K, theta, got):
    """The replay described at the top, over all lists of a call; returns the pool positions of the GPU's lists."""
    gidx, gval, gpen, gild = got
    n, N = ids.shape
    pos = _positions(ids, gidx)
    M = np.array([int(R.candidates(ids[r], vals[r]).sum()) for r in range(n)])
    T = (pos >= 0).sum(1)
    assert np.array_equal(T, np.minimum(K, M)), "%s: lists of %s picks, candidates %s" % (tag, T.tolist(), M.tolist())
    # val: the pool's bits at the returned id; empty slots -1 / 0 / 0
    want_val = np.where(pos >= 0, np.take_along_axis(vals, np.maximum(pos, 0), axis=1), np.float32(0))
    assert np.array_equal(_bits(gval), _bits(want_val.astype(np.float32))), tag
    assert (_bits(gpen)[pos < 0] == 0).all() and (_bits(gval)[pos < 0] == 0).all()
    o64, p64, l64 = R.replay(ids, vals, z64, pos, theta, np.float64)
    o32, p32, l32 = R.replay(ids, vals, z32, pos, theta, np.float32)
    rows = np.arange(n)[:, None]
    cols = np.arange(K)[None, :]
    pick64 = o64[rows, cols, np.maximum(pos, 0)]
    with np.errstate(all="ignore"):
        best64 = np.where(pos >= 0, np.nanmax(np.where(np.isnan(o64), -np.inf, o64), axis=2), np.nan)
    gap = float(np.nanmax(best64 - pick64, initial=0.0))
    d_o, a_o = _allowance(o64, o32)
    d_p, a_p = _allowance(p64, p32)
    d_l, a_l = _allowance(l64, l32)
    g_p = float(np.abs(gpen.astype(np.float64) - p64).max())
    g_l = float(np.abs(gild.astype(np.float64) - l64).max()) if gild is not None else 0.0
    print("%s: obj float32 deviation %.3e / allowance %.3e / GPU's pick below the float64 best by %.3e" % (tag, d_o, a_o, gap))
    print("%s: pen float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (tag, d_p, a_p, g_p))
    print("%s: ild float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (tag, d_l, a_l, g_l))
    assert not np.isnan(pick64[pos >= 0]).any()
    assert gap <= a_o and g_p <= a_p and g_l <= a_l, tag
    return pos


# ---- shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", S.SPACES)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("k,d", [(7, 15), (16, 12), (17, 16), (64, 64)])
def test_shapes_spaces_pools_and_thetas(k, d, dtype, space):
    """Widths below, at and above 16, odd ones included; pools of one item, below, at and above a wave and 256 = one slot of every
    thread; K = 1, 20 and the whole pool; 33 lists per call and the first of them alone."""
    I = 300
    t, z = _case(I, k, d, dtype)
    e, m = _vbpr(t, dtype), _bprmf(t)
    rn = e.sim_rnorm(space)
    for N in NS:
        ids, vals = _pools(33, I, N, seed=N + k)
        for K in sorted({1, min(20, N), N}):
            for theta in THETAS:
                tag = "k=%d d=%d %s %s N=%d K=%d theta=%g" % (k, d, dtype, space, N, K, theta)
                got = _call(e, space, rn, ids, vals, K, theta)
                pos = _check(tag, ids, vals, z[space][0], z[space][1], K, theta, got)
                one = _call(e, space, rn, ids[:1], vals[:1], K, theta)                        # n = 1: the grouped call's row
                assert all(np.array_equal(_bits(a[:1]), _bits(b)) for a, b in zip(got, one)), tag
                if theta == 0.0:
                    assert np.array_equal(got[0], ids[:, :K]) and np.array_equal(_bits(got[1]), _bits(vals[:, :K])), tag
                if K == N:
                    assert (np.sort(pos, axis=1) == np.arange(N)).all(), tag
                if space == "latent" and N in (20, 256):                                       # a BPRMF handle: the same Gi
                    rm = m.sim_rnorm("latent")
                    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, _call(m, "latent", rm, ids, vals, K, theta)))
    for eng in (e, m):
        eng.sync_check()
        eng.close()


@pytest.mark.parametrize("n", [1, 33])
def test_the_big_pool_reads_its_rows_from_memory(n):
    """N = 1024, K = 20, w = 128 (both, k = d = 64): 1024 rows of 129 floats are 516 KiB, far beyond a workgroup's LDS -- every
    round re-reads the candidates' rows from memory.  Four slots per thread."""
    I = 1100
    t, z = _case(I, 64, 64, "bf16")
    e = _vbpr(t, "bf16")
    rn = e.sim_rnorm("both")
    ids, vals = _pools(n, I, 1024, seed=5)
    for theta in THETAS:
        got = _call(e, "both", rn, ids, vals, 20, theta)
        _check("N=1024 n=%d theta=%g" % (n, theta), ids, vals, z["both"][0], z["both"][1], 20, theta, got)
        if theta == 0.0:
            assert np.array_equal(got[0], ids[:, :20])
    e.sync_check()
    e.close()


# ---- exact: the two row forms, calls, positions, neighbours --------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k,d", [("bf16", 16, 12), ("fp32", 7, 15), ("bf16", 64, 64)])
def test_a_lists_bits_do_not_depend_on_the_call_or_the_row_form(monkeypatch, dtype, k, d):
    I = 300
    t, z = _case(I, k, d, dtype)
    e = _vbpr(t, dtype)
    for space in S.SPACES:
        rn = e.sim_rnorm(space)
        for N, K, theta in ((70, 20, 0.3), (256, 256, 1.0), (65, 1, 0.3), (64, 64, 0.0)):
            ids, vals = _pools(33, I, N, seed=N + 1, short=((4, 0), (9, 1), (17, N // 2)))
            got = _call(e, space, rn, ids, vals, K, theta)
            _check("forms %s %s N=%d" % (dtype, space, N), ids, vals, z[space][0], z[space][1], K, theta, got)
            same = lambda a, b: all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
            assert same(got, _call(e, space, rn, ids, vals, K, theta)), "two calls differ"
            perm = np.random.RandomState(N).permutation(33)
            shuf = _call(e, space, rn, ids[perm], vals[perm], K, theta)
            assert same([g[perm] for g in got], shuf), "a list's bits depend on its position"
            for r in (0, 4, 32):
                assert same([g[r:r + 1] for g in got], _call(e, space, rn, ids[r:r + 1], vals[r:r + 1], K, theta)), "single list %d" % r
            no_ild = _call(e, space, rn, ids, vals, K, theta, want_ild=False)                     # ild == NULL: the rest unchanged
            assert same(got[:3], no_ild[:3])
            with monkeypatch.context() as mp:                                                      # the global-row form of the same pools
                mp.setenv("BPRX_DIVERSIFY_ROWS", "global")
                assert same(got, _call(e, space, rn, ids, vals, K, theta)), "the row forms differ (%s, N=%d)" % (space, N)
    e.sync_check()
    e.close()


def test_short_pools_fill_only_their_candidates():
    I, N = 300, 70
    t, z = _case(I, 16, 12, "bf16")
    e = _vbpr(t, "bf16")
    rn = e.sim_rnorm("visual")
    short = ((0, 0), (1, 1), (2, 2), (3, 19), (4, 20), (5, 21), (6, 69))
    ids, vals = _pools(8, I, N, seed=9, short=short)
    for K in (1, 20, 70):
        for theta in THETAS:
            gidx, gval, gpen, gild = got = _call(e, "visual", rn, ids, vals, K, theta)
            _check("short K=%d theta=%g" % (K, theta), ids, vals, z["visual"][0], z["visual"][1], K, theta, got)
            for r, M in short:
                T = min(K, M)
                assert (gidx[r, T:] == -1).all() and (_bits(gval[r, T:]) == 0).all() and (_bits(gpen[r, T:]) == 0).all()
                assert (gidx[r, :T] >= 0).all() and np.isfinite(gval[r, :T]).all()
                assert T >= 2 or _bits(gild[r:r + 1])[0] == 0
    e.sync_check()
    e.close()


@pytest.mark.parametrize("space", S.SPACES)
def test_of_twins_the_earlier_in_the_pool_is_picked_first(space):
    I, N = 300, 64
    t, z = _case(I, 16, 12, "bf16", special=True)
    e = _vbpr(t, "bf16")
    rn = e.sim_rnorm(space)
    ids, vals = _pools(6, I, N, seed=11)
    for r in range(6):                                             # both twins in every pool, 19 before 7 in the odd rows
        keep = [i for i in ids[r] if i not in (7, 19)][:N - 2]
        a, b = (7, 19) if r % 2 == 0 else (19, 7)
        ids[r] = np.array(keep[:r * 3] + [a] + keep[r * 3:r * 3 + 5] + [b] + keep[r * 3 + 5:], np.int32)
    for theta in (0.3, 1.0):                                       # (theta = 1: the twins' objectives are bit-equal at every step)
        got = _call(e, space, rn, ids, vals, N, theta)
        _check("twins %s theta=%g" % (space, theta), ids, vals, z[space][0], z[space][1], N, theta, got)
        for r in range(6):
            order = got[0][r].tolist()
            first, second = ((7, 19) if r % 2 == 0 else (19, 7))
            assert order.index(first) < order.index(second), (r, theta)
            assert abs(float(got[2][r, order.index(second)]) - 1.0) <= 1e-5      # the twin of a pick is wholly redundant
    e.sync_check()
    e.close()


def test_n_zero_writes_nothing():
    t, _ = _case(300, 16, 12, "bf16")
    e = _vbpr(t, "bf16")
    rn = e.sim_rnorm("both")
    lib = _ffi.lib()
    buf = torch.full((GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    bi = torch.full((GUARD,), -777, dtype=torch.int32, device="cuda")
    p = lambda x: x.data_ptr()
    assert lib.bprx_diversify(e.h, 2, p(rn), 0, 20, p(bi), p(buf), 5, 0.5, p(bi), p(buf), p(buf), p(buf), None) == 0
    assert lib.bprx_diversify(e.h, 2, p(rn), 0, 20, None, None, 5, 0.5, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (buf == PATTERN).all() and (bi == -777).all()
    out = e.diversify("both", rn, torch.zeros((0, 20), dtype=torch.int32, device="cuda"), torch.zeros((0, 20), device="cuda"), 5, 0.5)
    assert [tuple(o.shape) for o in out] == [(0, 5), (0, 5), (0, 5), (0,)]
    e.sync_check()
    e.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,form", [("sgd", None), ("adam_tf23", "lazy"), ("adam_tf23", "sweep")])
def test_the_call_leaves_the_state_alone(monkeypatch, opt, form):
    """Tables and Adam slots are bit-identical before and after the calls, and a 6-step run with them between steps 3 and 4 ends
    bit-identical to a run without them (duplicate-free batches: the step itself is then free of atomic-order noise)."""
    t = _tables(300, 600, 16, 12, 128, 100, "bf16", seed=17)
    batches = _unique_batches(300, 600, 64, 6, seed=18)
    ids, vals = (torch.as_tensor(x, device="cuda") for x in _pools(33, 600, 70, seed=19))
    lib = _ffi.lib()
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
                rn = [e.sim_rnorm(space) for space in S.SPACES]
                out = [torch.empty((33, 20), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.float32)]
                ild = torch.empty(33, device="cuda")
                torch.cuda.synchronize()
                held = lib.bprx_live_device_allocs()
                for q in range(3):
                    rc = lib.bprx_diversify(e.h, q, rn[q].data_ptr(), 33, 70, ids.data_ptr(), vals.data_ptr(), 20, 0.3,
                                            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ild.data_ptr(), None)
                    assert rc == 0
                torch.cuda.synchronize()
                assert lib.bprx_live_device_allocs() == held      # the calls allocated nothing
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


def test_a_pending_dense_update_is_settled_first(monkeypatch):
    """Right after a step that was not asked for its loss (its E|Bp update is still pending): the call sees the tables of a handle
    that never defers."""
    import test_gpu_dense_defer as dd
    ea, eb = dd._pair(monkeypatch, 256, 20, "bf16", "sgd")
    for s in range(2):
        b = dd._batch(300 + s)
        ea.step(*b, want_loss=False); eb.step(*b, want_loss=False)
    assert ea.dense_pending() and not eb.dense_pending()
    rn_b = eb.sim_rnorm("both")
    ids, vals = (torch.as_tensor(x, device="cuda") for x in _pools(9, ea.I, 64, seed=21))
    got = ea.diversify("both", rn_b, ids, vals, 20, 0.5)           # (the call itself meets the pending update)
    assert not ea.dense_pending()
    want = eb.diversify("both", rn_b, ids, vals, 20, 0.5)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(ea.sim_rnorm("both"), rn_b)
    dd._same_tables(ea, eb, "after the call")
    dd._close(ea, eb)


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable_and_no_allocation_behind():
    import test_gpu_acf as ga
    from acf_ref import random_tables
    from fashionvisualexpl_recommend_amd.engine import Engine
    lib = _ffi.lib()
    gc.collect()
    live = lib.bprx_live_device_allocs()
    I, N, K, n = 80, 20, 5, 6
    t = _tables(50, I, 16, 12, 256, 200, "bf16", seed=63)
    e, f8, m = _vbpr(t, "bf16"), _vbpr(t, "fp8"), _bprmf(t)
    unbound = Engine(model="vbpr", num_users=50, num_items=I, embed_k=16, embed_d=12, feat_dim=256, feat_dtype="bf16", optimizer="sgd",
                     max_batch=64)
    rs = np.random.RandomState(64)
    acf = ga._engine(random_tables(rs, 12, I, 16, 128, 64, 64, scale=10.0), ga._features(rs, I, 9, 128, "fp32"),
                     ga._lists(rs, 12, I, rs.randint(0, 15, 12)))
    ids_h, vals_h = _pools(n, I, N, seed=65)
    ids, vals = torch.as_tensor(ids_h, device="cuda"), torch.as_tensor(vals_h, device="cuda")
    rn = e.sim_rnorm("both")
    held = lib.bprx_live_device_allocs()
    good = [x.cpu().numpy() for x in e.diversify("both", rn, ids, vals, K, 0.5)]
    oi = torch.full((n * K + GUARD,), -777, dtype=torch.int32, device="cuda")
    ov, op, ol = (torch.full((n * K + GUARD,), PATTERN, dtype=torch.float32, device="cuda") for _ in range(3))

    def usable():
        again = [x.cpu().numpy() for x in e.diversify("both", rn, ids, vals, K, 0.5)]
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(good, again))
        e.sync_check()

    p = lambda x: None if x is None else x.data_ptr()
    call = lambda h, space=2, r=rn, nn=n, NN=N, pi=ids, pv=vals, KK=K, th=0.5, a=oi, b=ov, c=op, l=ol: lib.bprx_diversify(
        h, space, p(r), nn, NN, p(pi), p(pv), KK, th, p(a), p(b), p(c), p(l), None)
    assert call(None) == _ffi.E_INVALID
    bad = [lambda: call(e.h, r=None), lambda: call(e.h, pi=None), lambda: call(e.h, pv=None),          # null pointers
           lambda: call(e.h, a=None), lambda: call(e.h, b=None), lambda: call(e.h, c=None),
           lambda: call(e.h, space=3), lambda: call(e.h, space=-1),                                    # unknown spaces
           lambda: call(e.h, nn=-1), lambda: call(e.h, nn=1 << 31),                                    # ranges
           lambda: call(e.h, KK=0), lambda: call(e.h, KK=-3), lambda: call(e.h, KK=N + 1), lambda: call(e.h, NN=1025, KK=5),
           lambda: call(e.h, NN=0, KK=0), lambda: call(e.h, NN=0, KK=1),
           lambda: call(e.h, th=-0.01), lambda: call(e.h, th=1.01), lambda: call(e.h, th=float("nan")),
           lambda: call(e.h, th=float("inf"))]
    for q, c in enumerate(bad):
        assert c() == _ffi.E_INVALID, q
        assert lib.bprx_last_error(e.h).decode().startswith("diversify"), q
    torch.cuda.synchronize()
    assert (oi == -777).all() and all((x == PATTERN).all() for x in (ov, op, ol))      # no rejected call wrote anything
    usable()
    assert call(e.h, l=None) == 0 and call(e.h, th=0.0) == 0 and call(e.h, th=1.0) == 0        # ild may be NULL; the ends of [0, 1]
    # handles of the wrong kind, fp8 in a space that reads P, unbound tables
    for eng, spaces, code in ((m, ("visual", "both"), _ffi.E_INVALID), (f8, ("visual", "both"), _ffi.E_INVALID),
                              (acf, S.SPACES, _ffi.E_INVALID), (unbound, S.SPACES, _ffi.E_STATE)):
        for space in spaces:
            with pytest.raises(_ffi.BprxError) as err:
                eng.diversify(space, rn, ids, vals, K, 0.5)
            assert err.value.code == code, (space, code)
    assert "fp8" in lib.bprx_last_error(f8.h).decode()
    with pytest.raises(ValueError):
        e.diversify("both", rn, ids.long(), vals, K, 0.5)             # the pools are int32 / fp32
    # every handle goes on working: fp8 and BPRMF in the latent space give the bits of the bf16 handle (the same Gi)
    rl = e.sim_rnorm("latent")
    lat = [x.cpu().numpy() for x in e.diversify("latent", rl, ids, vals, K, 0.5)]
    for eng in (f8, m):
        other = [x.cpu().numpy() for x in eng.diversify("latent", eng.sim_rnorm("latent"), ids, vals, K, 0.5)]
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(lat, other))
    assert acf.score_block(0, 12).shape == (12, I)
    usable()
    # an id >= num_items: clamped, no fault, reported by sync_check; the handle stays usable
    wild = ids.clone()
    wild[2, 3] = I + 12345
    out = e.diversify("both", rn, wild, vals, N, 0.5)
    torch.cuda.synchronize()
    assert sorted(out[0][2].tolist()) == sorted(wild[2].tolist())       # the returned id is the pool's
    with pytest.raises(_ffi.BprxError) as err:
        e.sync_check()
    assert err.value.code == _ffi.E_RANGE
    usable()
    assert lib.bprx_live_device_allocs() == held
    for eng in (e, f8, m, unbound, acf):
        eng.close()
    assert lib.bprx_live_device_allocs() == live


# ---- model ---------------------------------------------------------------------------------------------------------------------
def _diverse_text(labels, res):
    out, oi = io.StringIO(), io.StringIO()
    ranking.write_diverse(out, oi, labels, *res)
    return out.getvalue(), oi.getvalue()


@pytest.mark.parametrize("space", [None, "latent", "both"])
def test_model_recommend_diverse(space):
    m, raw = _model(diversify=0.4, diversify_pool=30)                  # VBPR, bf16, U = 130, I = 60, k = 8, d = 20, top_k = 20
    e, ev = m.engine, m.evaluator
    U, I, K, N = 130, 60, 20, 30
    ev.user_block = 48                                                 # three blocks of users
    name = "visual" if space is None else space
    assert m.diversify_theta == 0.4 and m.diversify_pool == 30 and m.similar_space == "visual"
    ids, vals, pen, ild = m.recommend_diverse(space=space)
    assert ids.shape == vals.shape == pen.shape == (U, K) and ild.shape == (U,) and ids.dtype == np.int64
    # the pools the lists were picked from: the model's own top-30 (train items masked), as store_recommendation ranks them
    ev._metrics_device_csr()
    pi, pv, _ = ranking.rank_rows(ev._topk(0, U), e.score_block(0, U), N)
    t = {n: e.t[n] for n in ("Gi", "F", "E", "Bp")}
    z64, z32 = (S.item_vectors(t, name, "bf16", dt) for dt in (torch.float64, torch.float32))
    _check("recommend_diverse %s" % name, pi.astype(np.int32), pv, z64, z32, K, 0.4, (ids, vals, pen, ild))
    for u in range(U):
        assert not set(ids[u].tolist()) & set(m.data.training_list[u])
    assert (pen[:, 0] == 0).all() and (ild > 0).all() and not np.array_equal(ids, pi[:, :K])
    same = lambda a, b: all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    pick = [129, 0, 50, 50, 47, 48]
    assert same(m.recommend_diverse(pick, space=space), [x[pick] for x in (ids, vals, pen, ild)])
    plain = m.recommend_diverse(theta=0.0, space=space)                # theta = 0: the plain lists
    assert np.array_equal(plain[0], pi[:, :K]) and np.array_equal(_bits(plain[1]), _bits(pv[:, :K]))
    assert m.recommend_diverse([], space=space)[0].shape == (0, K)
    assert m.recommend_diverse([3], k=100, pool=100, space=space)[0].shape == (1, I)              # cut to the catalogue
    for bad in (dict(k=31), dict(pool=1025), dict(theta=1.5), dict(theta=-0.1), dict(users=[U])):
        with pytest.raises(ValueError):
            m.recommend_diverse(**bad)
    ev.force_host = True
    with pytest.raises(ValueError, match="--diversify"):
        m.recommend_diverse()
    ev.force_host = False
    ev.k = 2000
    with pytest.raises(ValueError, match="--diversify"):
        m.recommend_diverse()
    e.sync_check()
    e.close()


# ---- files ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec,space", [("vbpr", None), ("bprmf", None), ("vbpr", "both")])
def test_cli_writes_div_files_next_to_unchanged_recommendations(tmp_path, rec, space):
    from fashionvisualexpl_recommend_amd import train_rec
    U, Inum, top_k, pool = 30, 60, 10, 25
    tr, va, te = synth.make_interactions(U, Inum, per_user=8, seed=53)
    synth.write_dataset(str(tmp_path), "toy", tr, va, te, Inum, features=synth.make_features(Inum, 32, seed=55) if rec == "vbpr" else None)
    rows = [("new shopper", 3), ("b", 7), ("new shopper", 9), ("c 3", 5), ("c 3", 6), ("new shopper", 40), ("c 3", 5)]
    (tmp_path / "new.tsv").write_text("".join("%s\t%d\n" % r for r in rows))
    # --batch_size 1: a step adds at most one term to a gradient row, so runs of the same seed agree bit for bit
    common = ["--rec", rec, "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--reg", "0.01", "--top_k", str(top_k), "--lr", "0.01", "--optimizer", "sgd"]
    div = ["--diversify", "0.5", "--diversify_pool", str(pool)] + (["--similar_space", space] if space else [])
    new = ["--new_users", str(tmp_path / "new.tsv"), "--fold_steps", "9", "--fold_negatives", "3"]
    runs = [[], div, new, div + new]
    res = [str(tmp_path / ("res%d" % q)) for q in range(4)]
    for r, extra in zip(res, runs):
        train_rec.train(common + ["--results_root", r] + extra)
    m = train_rec._last_model                                          # (of the last run: it holds the last epoch's tables)
    rdir = [os.path.join(r, "rec_results", "toy", rec) for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] + files[2] if "div-" in f]
    assert [f for f in files[1] if "div-" not in f] == files[0] and [f for f in files[3] if "div-" not in f] == files[2]
    base = [f for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(base) == 2
    read = lambda q, f: open(os.path.join(rdir[q], f), "rb").read()
    for f in base:
        for q in (1, 2, 3):                                            # the catalogue's files: the bytes of the run without the flag
            assert read(0, f) == read(q, f), (f, q)
        nu = f.replace("recs-", "new-user-recs-", 1)
        assert read(2, nu) == read(3, nu)
        names = [os.path.basename(x) for x in ranking.div_paths(f) + ranking.div_paths(nu)]
        assert all(x in files[3] for x in names) and all(x in files[1] for x in names[:2]) and not [x for x in names[2:] if x in files[1]]
        assert read(1, names[0]) == read(3, names[0]) and read(1, names[1]) == read(3, names[1])
        got = [l.split("\t") for l in read(3, names[0]).decode().splitlines()]
        plain = [l.split("\t") for l in read(0, f).decode().splitlines()]
        assert len(got) == U * top_k and all(len(r) == 4 for r in got) and [r[0] for r in got] == [r[0] for r in plain]
        for u in range(U):
            blk = got[u * top_k:(u + 1) * top_k]
            assert len({r[1] for r in blk}) == top_k and not {int(r[1]) for r in blk} & set(tr[u])
            assert blk[0][1:3] == plain[u * top_k][1:3] and float(blk[0][3]) == 0.0               # the best item leads both lists
            assert all(-1.0001 <= float(r[3]) <= 1.0001 for r in blk)
        il = [l.split("\t") for l in read(3, names[1]).decode().splitlines()]
        assert [r[0] for r in il] == [str(u) for u in range(U)] and all(0.0 <= float(r[1]) <= 2.0001 for r in il)
        gn = [l.split("\t") for l in read(3, names[2]).decode().splitlines()]
        assert [r[0] for r in gn] == [lab for lab in ("new shopper", "b", "c 3") for _ in range(top_k)] and all(len(r) == 4 for r in gn)
        assert [l.split("\t")[0] for l in read(3, names[3]).decode().splitlines()] == ["new shopper", "b", "c 3"]
    # the rows of the last epoch's files are the model's own lists
    last = [f for f in base if f.startswith("recs-")][0]
    want, want_ild = _diverse_text(range(U), m.recommend_diverse())
    p_recs, p_ild = (os.path.basename(x) for x in ranking.div_paths(last))
    assert read(3, p_recs).decode() == want and read(3, p_ild).decode() == want_ild
    labels, lists = train_rec.read_new_users(str(tmp_path / "new.tsv"))
    want, want_ild = _diverse_text(labels, m.recommend_new_users(lists, diversify=0.5, steps=9, negatives=3, seed=0))
    p_recs, p_ild = (os.path.basename(x) for x in ranking.div_paths(last.replace("recs-", "new-user-recs-", 1)))
    assert read(3, p_recs).decode() == want and read(3, p_ild).decode() == want_ild
    m.engine.close()
