"""'Because you own X' on the MI355X: bprx_because against the float64 restatement (tests/because_ref.py), the model methods on top
of it and the because-* files of train_rec --because.

A top-L choice is discontinuous, so lists are never compared across precisions and no near-tie is left out: the GPU's OWN picks
are replayed in float64.  At each rank the float64 cosine of the GPU's pick must lie within the allowance of the largest float64
cosine among the entries not yet picked, and out_cos within the allowance of the float64 value of its entry.

Allowance (the rule of tests/test_gpu_diversify.py): 32 x the max-abs deviation of the FLOAT32 restatement from the float64 one over
the case, never below one float32 ulp of the largest magnitude.  Every comparison prints its triple (float32 deviation / allowance
/ GPU deviation).  What is exact is checked exactly.

Sizes the kernel really uses (csrc/bprx_because.hip, the launch rule at its end): a history tile holds 64 entries up to w = 123
and 32 at w = 128 (both, k = d = 64; a tile takes at most half the LDS), so histories of 31, 32, 33, of 63, 64, 65 and of 255, 256,
257 entries lie around one, two, four and eight tiles.  A list is cut into chunks of KC slots where the LDS rows demand it:
w = 128: KC = 86 / 77 / 45 for L = 1 / 5 / 32; w = 64 (latent or visual, k = d = 64): KC = 59 for L = 32 (132 for L = 5); the narrower
cases never cut K <= 65 (KC >= 83).  test_lists_around_a_chunk_of_slots runs K = KC - 1, KC, KC + 1 for each of the four."""
import gc
import io
import os

import numpy as np
import pytest
import torch

import because_ref as R
import similar_ref as S
from fashionvisualexpl_recommend_amd import _ffi, ranking, synth
from test_gpu_diversify import _allowance, _case
from test_gpu_feat_explain import _bits, _tables, _vbpr
from test_gpu_new_items import GUARD, PATTERN, _cli_dataset, _model, _new_rows
from test_gpu_similar import FEAT_D, _bprmf

pytestmark = pytest.mark.gpu

HLENS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 31, 32, 33)


def _hists(n, I, seed, lens=HLENS):
    """n ragged histories of distinct catalogue ids (a position is then known by its id), lengths cycling through `lens`."""
    rs = np.random.RandomState(seed)
    return [rs.permutation(I)[:lens[r % len(lens)]].astype(np.int32) for r in range(n)]


def _lists(hists, I, K, seed, nq=None):
    """[n, K] list entries: random items (rows of a table of nq new items), every seventh slot empty; catalogue items: slot 0 is an
    item of the list's own history wherever K > 1 or the row is odd, so that the item itself has to be skipped."""
    rs = np.random.RandomState(seed)
    n = len(hists)
    li = rs.randint(0, I if nq is None else nq, (n, K)).astype(np.int32)
    li[rs.random_sample((n, K)) < 1.0 / 7] = -1
    if nq is None:
        for r, h in enumerate(hists):
            if len(h) and (K > 1 or r % 2):
                li[r, 0] = h[len(h) // 2]
    return li


def _csr(hists):
    ptr = np.zeros(len(hists) + 1, np.int64)
    np.cumsum([len(h) for h in hists], out=ptr[1:])
    items = np.concatenate([np.asarray(h, np.int32) for h in hists] + [np.zeros(1, np.int32)])
    return torch.as_tensor(ptr, device="cuda"), torch.as_tensor(items, device="cuda")


def _call(e, space, rn, lists, hists, L, Pq=None, rq=None, want_cnt=True):
    """One bprx_because call into guarded buffers: numpy item [n, K, L], cos [n, K, L], cnt [n, K] (None without)."""
    lib = _ffi.lib()
    n, K = lists.shape
    li = torch.as_tensor(np.ascontiguousarray(lists, dtype=np.int32), device="cuda")
    ptr, items = _csr(hists)
    bi = torch.full((n * K * L + GUARD,), -777, dtype=torch.int32, device="cuda")
    bc = torch.full((n * K * L + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    bn = torch.full((n * K + GUARD,), -777, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    nq = e.I if Pq is None else int(Pq.shape[0])
    rc = lib.bprx_because(e.h, _ffi.SIM_SPACE[space], p(Pq), nq, p(rq), p(rn), n, K, p(li), p(ptr), p(items), L, p(bi), p(bc),
                          p(bn) if want_cnt else None, None)
    _ffi.check(e.h, rc)
    torch.cuda.synchronize()
    assert (bi[n * K * L:] == -777).all() and (bc[n * K * L:] == PATTERN).all(), "wrote behind an output"
    assert (bn[n * K if want_cnt else 0:] == -777).all(), "wrote behind cnt"
    return (bi[:n * K * L].view(n, K, L).cpu().numpy(), bc[:n * K * L].view(n, K, L).cpu().numpy(),
            bn[:n * K].view(n, K).cpu().numpy() if want_cnt else None)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b) if x is not None and y is not None)


def _check(tag, lists, hists, z64, z32, L, got, zq64=None, zq32=None):
    """The replay described at the top, over every slot of a call."""
    item, cos, cnt = got
    n, K = lists.shape
    _, _, cnt64, _, all64 = R.because_lists(lists, hists, z64, L, np.float64, zq64)
    _, _, _, _, all32 = R.because_lists(lists, hists, z32, L, np.float32, zq32)
    if cnt is not None:
        assert np.array_equal(cnt, cnt64), "%s: cnt" % tag
    T = np.minimum(L, cnt64)
    filled = np.arange(L)[None, None, :] < T[:, :, None]
    assert ((item >= 0) == filled).all(), "%s: %d slots filled or empty against min(L, M)" % (tag, int(((item >= 0) != filled).sum()))
    assert (item[~filled] == -1).all() and (_bits(cos)[~filled] == 0).all(), "%s: tails hold -1 / 0.0f" % tag
    pos = np.full(item.shape, -1, np.int64)                              # the picks' history positions
    for r, h in enumerate(hists):
        where = np.full(int(max(z64.shape[0], 1)), -1, np.int64)
        where[np.asarray(h, np.int64)] = np.arange(len(h))
        pos[r] = np.where(item[r] >= 0, where[np.maximum(item[r], 0)], -1)
    assert ((pos >= 0) == filled).all(), "%s: a returned id is not in its history" % tag
    d_c, a_c = _allowance(all64, all32)
    work = np.where(np.isnan(all64), -np.inf, all64)
    gap = g_c = 0.0
    for s in range(L):
        on = pos[:, :, s] >= 0
        if not on.any():
            break
        pick = np.take_along_axis(work, np.maximum(pos[:, :, s:s + 1], 0), axis=2)[:, :, 0]
        assert np.isfinite(pick[on]).all(), "%s: rank %d picks no candidate, or one picked before" % (tag, s)
        gap = max(gap, float((work.max(axis=2)[on] - pick[on]).max()))
        g_c = max(g_c, float(np.abs(cos[:, :, s].astype(np.float64) - pick)[on].max()))
        rr, qq = np.nonzero(on)
        work[rr, qq, pos[rr, qq, s]] = -np.inf
    print("%s: cos float32 deviation %.3e / allowance %.3e / GPU deviation %.3e / GPU's pick below the float64 best by %.3e"
          % (tag, d_c, a_c, g_c, gap))
    assert gap <= a_c and g_c <= a_c, tag
    return pos


# ---- shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", S.SPACES)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("k,d", [(7, 15), (16, 12), (17, 16), (64, 64)])
def test_shapes_spaces_lists_and_tops(k, d, dtype, space):
    """Widths below, at and above 16, odd ones included; 33 lists per call with ragged histories of 0 .. 257 entries (HLENS); K = 1, 20, 65
    and L = 1, 5, 32.  The first list alone and one column as a K = 1 call return the grouped call's bits."""
    I = 300
    t, z = _case(I, k, d, dtype)
    e, m = _vbpr(t, dtype), _bprmf(t)
    rn = e.sim_rnorm(space)
    hists = _hists(33, I, seed=k + d)
    for K in (1, 20, 65):
        lists = _lists(hists, I, K, seed=K + k)
        for L in (1, 5, 32):
            tag = "k=%d d=%d %s %s K=%d L=%d" % (k, d, dtype, space, K, L)
            got = _call(e, space, rn, lists, hists, L)
            _check(tag, lists, hists, z[space][0], z[space][1], L, got)
            assert _same([g[:1] for g in got], _call(e, space, rn, lists[:1], hists[:1], L)), tag         # n = 1
            assert _same([g[8:9] for g in got], _call(e, space, rn, lists[8:9], hists[8:9], L)), tag       # (257 entries)
            if K > 1:
                q = K // 3
                col = _call(e, space, rn, lists[:, q:q + 1].copy(), hists, L)                              # K = 1
                assert _same([g[:, q:q + 1] for g in got], col), tag
            assert _same(got[:2], _call(e, space, rn, lists, hists, L, want_cnt=False)[:2]), tag           # out_cnt == NULL
            if space == "latent" and K == 20:                                                              # a BPRMF handle: the same Gi
                assert _same(got, _call(m, "latent", m.sim_rnorm("latent"), lists, hists, L)), tag
    for eng in (e, m):
        eng.sync_check()
        eng.close()


def test_long_histories_walk_many_tiles():
    """I = 1600, histories of 600 and 1500 entries (19 and 47 tiles of 32) beside short ones, w = 128."""
    I = 1600
    t, z = _case(I, 64, 64, "bf16")
    e = _vbpr(t, "bf16")
    rn = e.sim_rnorm("both")
    hists = _hists(4, I, seed=3, lens=(600, 1500, 5, 0))
    lists = _lists(hists, I, 20, seed=4)
    for L in (5, 32):
        got = _call(e, "both", rn, lists, hists, L)
        _check("long L=%d" % L, lists, hists, z["both"][0], z["both"][1], L, got)
        assert _same([g[1:2] for g in got], _call(e, "both", rn, lists[1:2], hists[1:2], L))
    e.sync_check()
    e.close()


@pytest.mark.parametrize("space,L,KC", [("both", 1, 86), ("both", 5, 77), ("both", 32, 45), ("visual", 32, 59)])
def test_lists_around_a_chunk_of_slots(space, L, KC):
    """K = KC - 1, KC, KC + 1 (see the top): the slots' bits are those of the longest list, however the list is cut."""
    I = 300
    t, z = _case(I, 64, 64, "bf16")
    e = _vbpr(t, "bf16")
    rn = e.sim_rnorm(space)
    hists = _hists(9, I, seed=KC)
    lists = _lists(hists, I, 2 * KC + 1, seed=KC + 1)
    whole = _call(e, space, rn, lists, hists, L)                         # three chunks: KC, KC, 1
    _check("chunks %s L=%d K=%d" % (space, L, 2 * KC + 1), lists, hists, z[space][0], z[space][1], L, whole)
    for K in (KC - 1, KC, KC + 1):
        got = _call(e, space, rn, lists[:, :K].copy(), hists, L)
        assert _same([g[:, :K] for g in whole], got), (space, L, K)
    e.sync_check()
    e.close()


# ---- exact ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k,d", [("bf16", 16, 12), ("fp32", 7, 15), ("bf16", 64, 64)])
def test_the_cosine_has_the_bits_of_diversifys_penalty_and_of_the_swapped_pair(dtype, k, d):
    I, n = 300, 64
    t, _ = _case(I, k, d, dtype)
    e = _vbpr(t, dtype)
    rs = np.random.RandomState(k)
    a = rs.randint(0, I, n).astype(np.int32)
    b = ((a + 1 + rs.randint(0, I - 1, n)) % I).astype(np.int32)         # b != a
    for space in S.SPACES:
        rn = e.sim_rnorm(space)
        ab = _call(e, space, rn, a[:, None], [b[r:r + 1] for r in range(n)], 1)
        ba = _call(e, space, rn, b[:, None], [a[r:r + 1] for r in range(n)], 1)
        assert np.array_equal(ab[0][:, 0, 0], b) and np.array_equal(ba[0][:, 0, 0], a) and (ab[2] == 1).all()
        assert np.array_equal(_bits(ab[1]), _bits(ba[1])), "cos(i, l) != cos(l, i) in %s" % space
        pool = torch.as_tensor(np.stack([a, b], 1), device="cuda")
        val = torch.as_tensor(np.tile(np.array([2.0, 1.0], np.float32), (n, 1)), device="cuda")
        pen = e.diversify(space, rn, pool, val, 2, 0.5)[2].cpu().numpy()
        assert np.array_equal(_bits(ab[1][:, 0, 0]), _bits(pen[:, 1])), "bprx_diversify's pen differs in %s" % space
    e.sync_check()
    e.close()


@pytest.mark.parametrize("space", S.SPACES)
def test_twins_come_out_in_position_order_with_equal_bits(space):
    I = 300
    t, z = _case(I, 16, 12, "bf16", special=True)
    e = _vbpr(t, "bf16")
    rn = e.sim_rnorm(space)
    rs = np.random.RandomState(5)
    hists = []
    for r in range(8):                                             # both twins in every history, 19 before 7 in the odd rows
        h = [i for i in rs.permutation(I) if i not in (7, 19)][:10 + 9 * r]
        x, y = (7, 19) if r % 2 == 0 else (19, 7)
        hists.append(np.array(h[:r] + [x] + h[r:r + 4] + [y] + h[r + 4:], np.int32))
    lists = rs.randint(20, I, (8, 6)).astype(np.int32)
    item, cos, cnt = got = _call(e, space, rn, lists, hists, 32)
    _check("twins %s" % space, lists, hists, z[space][0], z[space][1], 32, got)
    seen = 0
    for r in range(8):
        first, second = (7, 19) if r % 2 == 0 else (19, 7)
        for q in range(6):
            row = item[r, q].tolist()
            if first in row and second in row:
                seen += 1
                assert row.index(second) == row.index(first) + 1, (r, q)
                assert _bits(cos[r, q])[row.index(first)] == _bits(cos[r, q])[row.index(second)]
            else:
                assert second not in row                           # (the later twin never gets in without the earlier)
    assert seen >= 8
    e.sync_check()
    e.close()


def test_repeated_ids_are_entries_of_their_own_and_the_item_itself_is_none():
    I = 300
    t, _ = _case(I, 16, 12, "bf16")
    e = _vbpr(t, "bf16")
    rn = e.sim_rnorm("both")
    hists = [np.array([4, 9, 4, 4, 9], np.int32), np.array([5, 5], np.int32), np.array([5], np.int32)]
    lists = np.array([[9, 4, 30], [5, 6, -1], [5, -1, 5]], np.int32)
    item, cos, cnt = _call(e, "both", rn, lists, hists, 4)
    assert cnt.tolist() == [[3, 2, 5], [0, 2, 0], [0, 0, 0]]
    assert item[0, 0].tolist() == [4, 4, 4, -1] and item[0, 1].tolist() == [9, 9, -1, -1] and item[1, 0].tolist() == [-1] * 4
    assert len(set(_bits(cos[0, 0, :3]).tolist())) == 1 and len(set(_bits(cos[0, 1, :2]).tolist())) == 1
    assert item[0, 2].tolist() in ([4, 4, 4, 9], [9, 9, 4, 4])    # five entries, two distinct cosines: the top 4, grouped by value
    assert item[1, 1].tolist() == [5, 5, -1, -1] and (item[2] == -1).all() and (_bits(cos[2]) == 0).all()
    e.sync_check()
    e.close()


def test_n_zero_writes_nothing():
    t, _ = _case(300, 16, 12, "bf16")
    e = _vbpr(t, "bf16")
    rn = e.sim_rnorm("both")
    lib = _ffi.lib()
    buf = torch.full((GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    bi = torch.full((GUARD,), -777, dtype=torch.int32, device="cuda")
    ptr = torch.zeros(1, dtype=torch.int64, device="cuda")
    p = lambda x: x.data_ptr()
    assert lib.bprx_because(e.h, 2, None, 300, None, p(rn), 0, 20, p(bi), p(ptr), p(bi), 5, p(bi), p(buf), p(bi), None) == 0
    assert lib.bprx_because(e.h, 2, None, 300, None, p(rn), 0, 20, None, None, None, 5, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (buf == PATTERN).all() and (bi == -777).all()
    out = e.because("both", rn, torch.zeros((0, 20), dtype=torch.int32, device="cuda"), (ptr, bi), 5)
    assert [tuple(o.shape) for o in out] == [(0, 20, 5), (0, 20, 5), (0, 20)]
    e.sync_check()
    e.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------
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
    hists = _hists(9, ea.I, seed=21, lens=(0, 3, 70))
    li = torch.as_tensor(_lists(hists, ea.I, 20, seed=22), device="cuda")
    got = ea.because("both", rn_b, li, _csr(hists), 5)             # (the call itself meets the pending update)
    assert not ea.dense_pending()
    want = eb.because("both", rn_b, li, _csr(hists), 5)
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
    I, K, L, n = 80, 6, 3, 5
    t = _tables(50, I, 16, 12, 256, 200, "bf16", seed=63)
    e, f8, m = _vbpr(t, "bf16"), _vbpr(t, "fp8"), _bprmf(t)
    unbound = Engine(model="vbpr", num_users=50, num_items=I, embed_k=16, embed_d=12, feat_dim=256, feat_dtype="bf16", optimizer="sgd",
                     max_batch=64)
    rs = np.random.RandomState(64)
    acf = ga._engine(random_tables(rs, 12, I, 16, 128, 64, 64, scale=10.0), ga._features(rs, I, 9, 128, "fp32"),
                     ga._lists(rs, 12, I, rs.randint(0, 15, 12)))
    hists = _hists(n, I, seed=65, lens=(0, 7, 70))
    li = torch.as_tensor(_lists(hists, I, K, seed=66), device="cuda")
    csr = ptr, items = _csr(hists)
    rn = e.sim_rnorm("both")
    P = e.project_rows(e._new_table(_new_rows(4, 256, 200, "bf16", seed=67)))
    rq, rv = e.sim_rnorm("visual", P), e.sim_rnorm("visual")
    torch.cuda.synchronize()
    held = lib.bprx_live_device_allocs()
    good = [x.cpu().numpy() for x in e.because("both", rn, li, csr, L)]
    assert lib.bprx_live_device_allocs() == held                    # the call allocated nothing
    oi = torch.full((n * K * L + GUARD,), -777, dtype=torch.int32, device="cuda")
    oc = torch.full((n * K * L + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    on = torch.full((n * K + GUARD,), -777, dtype=torch.int32, device="cuda")

    def usable():
        again = [x.cpu().numpy() for x in e.because("both", rn, li, csr, L)]
        assert _same(good, again)
        e.sync_check()

    p = lambda x: None if x is None else x.data_ptr()
    call = lambda h, space=2, Pq=None, nq=I, q=None, r=rn, nn=n, KK=K, l=li, hp=ptr, hi=items, LL=L, a=oi, b=oc, c=on: lib.bprx_because(
        h, space, p(Pq), nq, p(q), p(r), nn, KK, p(l), p(hp), p(hi), LL, p(a), p(b), p(c), None)
    assert call(None) == _ffi.E_INVALID
    bad = [lambda: call(e.h, r=None), lambda: call(e.h, l=None), lambda: call(e.h, hp=None), lambda: call(e.h, hi=None),  # null pointers
           lambda: call(e.h, a=None), lambda: call(e.h, b=None),
           lambda: call(e.h, space=1, Pq=P, nq=4, q=None, r=rv),                                       # new rows without their norms
           lambda: call(e.h, space=3), lambda: call(e.h, space=-1),                                    # unknown spaces
           lambda: call(e.h, nn=-1), lambda: call(e.h, nn=1 << 31),                                    # ranges
           lambda: call(e.h, KK=0), lambda: call(e.h, KK=-3), lambda: call(e.h, KK=1025),
           lambda: call(e.h, LL=0), lambda: call(e.h, LL=-1), lambda: call(e.h, LL=33),
           lambda: call(e.h, space=2, Pq=P, nq=4, q=rq), lambda: call(e.h, space=0, Pq=P, nq=4, q=rq),  # new rows: visual only
           lambda: call(e.h, nq=I - 1), lambda: call(e.h, space=1, Pq=P, nq=-1, q=rq, r=rv)]           # nq
    for q, c in enumerate(bad):
        assert c() == _ffi.E_INVALID, q
        assert lib.bprx_last_error(e.h).decode().startswith("because"), q
    torch.cuda.synchronize()
    assert (oi == -777).all() and (oc == PATTERN).all() and (on == -777).all()      # no rejected call wrote anything
    usable()
    assert call(e.h, c=None) == 0 and call(e.h, q=rn) == 0                          # cnt may be NULL; rn_q may be given
    # L = 32 writes n * K * 32 entries: outputs of its own size (oi / oc hold n * K * L and were written past their end here once,
    # which faulted or not with where the allocator had put them)
    wi = torch.full((n * K * 32 + GUARD,), -777, dtype=torch.int32, device="cuda")
    wc = torch.full((n * K * 32 + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    assert call(e.h, LL=32, a=wi, b=wc) == 0
    torch.cuda.synchronize()
    assert (wi[n * K * 32:] == -777).all() and (wc[n * K * 32:] == PATTERN).all() and not (wi[:n * K * 32] == -777).any()
    assert call(e.h, space=1, Pq=P, nq=4, q=rq, r=rv, l=torch.zeros_like(li)) == 0
    # handles of the wrong kind, fp8 in a space that reads P, unbound tables
    for eng, spaces, code in ((m, ("visual", "both"), _ffi.E_INVALID), (f8, ("visual", "both"), _ffi.E_INVALID),
                              (acf, S.SPACES, _ffi.E_INVALID), (unbound, S.SPACES, _ffi.E_STATE)):
        for space in spaces:
            with pytest.raises(_ffi.BprxError) as err:
                eng.because(space, rn, li, csr, L)
            assert err.value.code == code, (space, code)
    assert "fp8" in lib.bprx_last_error(f8.h).decode()
    with pytest.raises(ValueError):
        e.because("both", rn, li.long(), csr, L)                    # the lists are int32
    with pytest.raises(ValueError):
        e.because("visual", rv, li, csr, L, Pq=P)                    # rows from outside come with their norms
    # every handle goes on working: fp8 and BPRMF in the latent space give the bits of the bf16 handle (the same Gi)
    lat = [x.cpu().numpy() for x in e.because("latent", e.sim_rnorm("latent"), li, csr, L)]
    for eng in (f8, m):
        assert _same(lat, [x.cpu().numpy() for x in eng.because("latent", eng.sim_rnorm("latent"), li, csr, L)])
    assert acf.score_block(0, 12).shape == (12, I)
    usable()
    # ids >= num_items, in a list and in a history: clamped, no fault, reported by sync_check; the handle stays usable
    wild = li.clone()
    wild[2, 3] = I + 12345
    out = e.because("both", rn, wild, csr, L)
    torch.cuda.synchronize()
    assert _same([np.delete(x.cpu().numpy(), 2, 0) for x in out], [np.delete(x, 2, 0) for x in good])   # the other lists: unchanged
    with pytest.raises(_ffi.BprxError) as err:
        e.sync_check()
    assert err.value.code == _ffi.E_RANGE
    usable()
    wild_items = items.clone()
    wild_items[int(ptr[1])] = I + 999                              # (list 1 owns 7 items: L = 32 names them all)
    out = e.because("both", rn, li, (ptr, wild_items), 32)
    torch.cuda.synchronize()
    assert (out[0][1] == I + 999).any()                            # the returned id is the history's
    with pytest.raises(_ffi.BprxError) as err:
        e.sync_check()
    assert err.value.code == _ffi.E_RANGE
    usable()
    assert lib.bprx_live_device_allocs() == held
    del P, rq, rv
    for eng in (e, f8, m, unbound, acf):
        eng.close()
    gc.collect()
    assert lib.bprx_live_device_allocs() == live


# ---- new items -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k,d", [("bf16", 16, 12), ("fp32", 7, 15), ("bf16", 64, 64)])
def test_rows_from_outside_the_catalogue(dtype, k, d):
    I, nq = 300, 37
    t, z = _case(I, k, d, dtype)
    e = _vbpr(t, dtype)
    Fn = _new_rows(nq, FEAT_D[dtype], 390, dtype, seed=k)
    zq = tuple(S.item_vectors(t, "visual", dtype, dt, F=Fn) for dt in (torch.float64, torch.float32))
    P = e.project_rows(e._new_table(Fn))
    rn, rq = e.sim_rnorm("visual"), e.sim_rnorm("visual", P)
    hists = _hists(33, I, seed=k + 1)
    for K, L in ((1, 32), (20, 5), (65, 1)):
        lists = _lists(hists, I, K, seed=K, nq=nq)
        got = _call(e, "visual", rn, lists, hists, L, P, rq)
        _check("new rows k=%d d=%d %s K=%d L=%d" % (k, d, dtype, K, L), lists, hists, z["visual"][0], z["visual"][1], L, got, *zq)
        assert np.array_equal(got[2], np.where(lists >= 0, np.array([len(h) for h in hists])[:, None], 0))   # nothing is skipped
        assert _same([g[:1] for g in got], _call(e, "visual", rn, lists[:1], hists[:1], L, P, rq))
    for space in ("latent", "both"):
        with pytest.raises(_ffi.BprxError) as err:
            e.because(space, e.sim_rnorm(space), torch.zeros((1, 1), dtype=torch.int32, device="cuda"), _csr(hists[:1]), 1, P, rq)
        assert err.value.code == _ffi.E_INVALID
    e.sync_check()
    e.close()


# ---- model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", [None, "latent", "both"])
def test_model_because(space):
    m, raw = _model()                                                  # VBPR, bf16, U = 130, I = 60, k = 8, d = 20, top_k = 20
    e = m.engine
    U, I = 130, 60
    name = "visual" if space is None else space
    rs = np.random.RandomState(7)
    users = np.repeat(rs.permutation(U)[:40], 5)
    items = rs.randint(0, I, users.size)
    hist, cos, count = m.because(users, items, 4, space)
    assert hist.shape == cos.shape == (200, 4) and count.shape == (200,) and hist.dtype == np.int64 and cos.dtype == np.float32
    tr = [list(dict.fromkeys(l)) for l in m.data.training_list]
    t = {n: e.t[n] for n in ("Gi", "F", "E", "Bp")}
    z64, z32 = (S.item_vectors(t, name, "bf16", dt) for dt in (torch.float64, torch.float32))
    lists = items.reshape(40, 5).astype(np.int32)
    hs = [np.array(tr[u], np.int32) for u in users[::5]]
    _check("model.because %s" % name, lists, hs, z64, z32, 4, (hist.reshape(40, 5, 4).astype(np.int32), cos.reshape(40, 5, 4),
                                                               count.reshape(40, 5).astype(np.int32)))
    for p in range(200):
        own = set(tr[users[p]])
        assert set(hist[p][hist[p] >= 0].tolist()) <= own - {int(items[p])} and count[p] == len(own - {int(items[p])})
    # any order of the pairs: each pair's row is the same
    perm = rs.permutation(200)
    assert _same(m.because(users[perm], items[perm], 4, space), [x[perm] for x in (hist, cos, count)])
    # histories of the caller's own
    mine = [[3, 4, 5], [], [9]]
    h2, c2, n2 = m.because([0, 0, 2, 1], [3, 7, 9, 2], 2, space, lists=mine)
    assert n2.tolist() == [2, 3, 0, 0] and set(h2[0].tolist()) == {4, 5} and (h2[2:] == -1).all() and (c2[2:] == 0).all()
    assert m.because([], [], 3, space)[0].shape == (0, 3)
    for bad in (dict(users=[U], items=[0]), dict(users=[0], items=[0], top=0), dict(users=[0], items=[0], top=33),
                dict(users=[0, 1], items=[0])):
        with pytest.raises(ValueError):
            m.because(**bad)
    m.evaluator.force_host = True
    with pytest.raises(ValueError, match="--because"):
        m.because([0], [1])
    m.evaluator.force_host = False
    e.sync_check()
    e.close()


def test_model_because_new():
    m, raw = _model()
    e = m.engine
    new_raw = synth.make_features(9, 128, seed=41) * 3.0
    rs = np.random.RandomState(8)
    users = np.repeat(rs.permutation(130)[:30], 3)
    rows = rs.randint(0, 9, users.size)
    hist, cos, count = m.because_new(new_raw, users, rows, 5)
    Fd = m.prepare_new_items(new_raw)
    assert _same((hist, cos, count), m.because_new(Fd, users, rows, 5))
    tr = [list(dict.fromkeys(l)) for l in m.data.training_list]
    t = {n: e.t[n] for n in ("Gi", "F", "E", "Bp")}
    z64, z32 = (S.item_vectors(t, "visual", "bf16", dt) for dt in (torch.float64, torch.float32))
    zq = tuple(S.item_vectors(t, "visual", "bf16", dt, F=Fd.float().cpu().numpy()) for dt in (torch.float64, torch.float32))
    _check("model.because_new", rows.reshape(30, 3).astype(np.int32), [np.array(tr[u], np.int32) for u in users[::3]], z64, z32, 5,
           (hist.reshape(30, 3, 5).astype(np.int32), cos.reshape(30, 3, 5), count.reshape(30, 3).astype(np.int32)), *zq)
    assert np.array_equal(count, [len(tr[u]) for u in users])
    with pytest.raises(ValueError):
        m.because_new(new_raw, [0], [9], 5)
    e.sync_check()
    e.close()


# ---- files ---------------------------------------------------------------------------------------------------------------------
def _expected(list_rows, hist, cos):
    """The because-rows of the pairs of a list file (rows already split into fields), as ranking.write_because writes them."""
    out = []
    for p, row in enumerate(list_rows):
        head = "\t".join(row[:3]) + "\t"
        if hist[p, 0] < 0:
            out.append(head + "-1\t-1\t0.0\n")
        for s in range(hist.shape[1]):
            if hist[p, s] < 0:
                break
            out.append(head + str(s) + "\t" + str(hist[p, s]) + "\t" + str(cos[p, s]) + "\n")
    return "".join(out)


@pytest.mark.parametrize("rec,dtype", [("vbpr", "bf16"), ("bprmf", "fp32")])
def test_cli_writes_because_files_next_to_unchanged_files(tmp_path, rec, dtype):
    from fashionvisualexpl_recommend_amd import train_rec
    U, top_k = 30, 10
    if rec == "vbpr":
        paths, n_new, _ = _cli_dataset(tmp_path, rec)
    else:
        tr, va, te = synth.make_interactions(U, 60, per_user=8, seed=53)
        synth.write_dataset(str(tmp_path), "toy", tr, va, te, 60)
    rows = [("new shopper", 3), ("b", 7), ("new shopper", 9), ("c 3", 5), ("c 3", 6), ("new shopper", 40), ("c 3", 5)]
    (tmp_path / "new.tsv").write_text("".join("%s\t%d\n" % r for r in rows))
    # --batch_size 1: a step adds at most one term to a gradient row, so runs of the same seed agree bit for bit
    common = ["--rec", rec, "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--reg", "0.01", "--top_k", str(top_k), "--lr", "0.01", "--optimizer", "sgd", "--dtype", dtype,
              "--new_users", str(tmp_path / "new.tsv"), "--fold_steps", "9", "--fold_negatives", "3", "--diversify", "0.5",
              "--diversify_pool", "25"]
    if rec == "vbpr":
        common += ["--feat_explain", "3", "--new_items"] + paths
    res = [str(tmp_path / ("res%d" % q)) for q in range(2)]
    train_rec.train(common + ["--results_root", res[0]])
    train_rec.train(common + ["--results_root", res[1], "--because", "3"])
    m = train_rec._last_model                                          # (of the last run: it holds the last epoch's tables)
    rdir = [os.path.join(r, "rec_results", "toy", rec) for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] if "because-" in f]
    assert [f for f in files[1] if "because-" not in f] == files[0]
    read = lambda q, f: open(os.path.join(rdir[q], f), "rb").read()
    for f in files[0]:                                                 # recs-*, new-user-recs-*, new-recs-*, expl-*, div-*: the same bytes
        if f.endswith(".tsv"):
            assert read(0, f) == read(1, f), f
    assert [f for f in files[0] if f.startswith(("expl-", "new-recs-"))] or rec == "bprmf"
    assert [f for f in files[0] if f.startswith("div-recs-")] and [f for f in files[0] if f.startswith("new-user-recs-")]
    base = [f for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(base) == 2
    kinds = ["recs-", "new-user-recs-"] + (["new-recs-"] if rec == "vbpr" else [])
    for f in base:
        for kind in kinds:
            lf = f.replace("recs-", kind, 1)
            bf = os.path.basename(ranking.because_paths(lf))
            assert bf in files[1] and not [x for x in files[1] if x.startswith("because-div") or x.startswith("div-because")]
            pairs = [l.split("\t") for l in read(1, lf).decode().splitlines()]
            got = [l.split("\t") for l in read(1, bf).decode().splitlines()]
            assert all(len(r) == 6 for r in got)
            assert list(dict.fromkeys(tuple(r[:3]) for r in got)) == [tuple(r) for r in pairs], bf      # every pair, in order
    # the rows of the last epoch's files are the model's own
    last = [f for f in base if f.startswith("recs-")][0]
    pairs = [l.split("\t") for l in read(1, last).decode().splitlines()]
    hist, cos, _ = m.because([int(r[0]) for r in pairs], [int(r[1]) for r in pairs], 3)
    assert read(1, os.path.basename(ranking.because_paths(last))).decode() == _expected(pairs, hist, cos)
    assert (hist[:, 0] >= 0).all()                                     # (every user owns something else than the recommended item)
    labels, lists = train_rec.read_new_users(str(tmp_path / "new.tsv"))
    nu = last.replace("recs-", "new-user-recs-", 1)
    pairs = [l.split("\t") for l in read(1, nu).decode().splitlines()]
    hist, cos, cnt = m.because([labels.index(r[0]) for r in pairs], [int(r[1]) for r in pairs], 3,
                               lists=[list(dict.fromkeys(l)) for l in lists])
    assert read(1, os.path.basename(ranking.because_paths(nu))).decode() == _expected(pairs, hist, cos)
    assert set(cnt.tolist()) == {3, 1, 2}                              # the file's histories, deduplicated ("c 3" repeats item 5)
    if rec == "vbpr":
        nr = last.replace("recs-", "new-recs-", 1)
        pairs = [l.split("\t") for l in read(1, nr).decode().splitlines()]
        hist, cos, _ = m.because_new(np.load(paths[0]), [int(r[0]) for r in pairs], [int(r[1]) for r in pairs], 3)
        assert read(1, os.path.basename(ranking.because_paths(nr))).decode() == _expected(pairs, hist, cos)
    m.engine.close()


def test_cli_grad_fashion_explains_its_top_k_lists(tmp_path):
    from fashionvisualexpl_recommend_amd import train_rec
    _cli_dataset(tmp_path, "grad_fashion")
    U, top_k = 30, 10
    train_rec.train(["--rec", "grad_fashion", "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "1", "--batch_size", "1",
                     "--embed_k", "16", "--embed_d", "8", "--embed_color", "4", "--embed_edges", "6", "--reg", "0.01", "--top_k",
                     str(top_k), "--lr", "0.01", "--results_root", str(tmp_path / "res"), "--because", "2", "--similar_space", "both"])
    m = train_rec._last_model
    rdir = os.path.join(str(tmp_path / "res"), "rec_results", "toy", "grad_fashion")
    last = [f for f in sorted(os.listdir(rdir)) if f.startswith("because-")]
    assert len(last) == 1 and [f for f in os.listdir(rdir) if f.startswith("best-because-")]
    ev, e = m.evaluator, m.engine
    ev._metrics_device_csr()
    ids, vals, _ = ranking.rank_rows(ev._topk(0, U), e.score_block(0, U), top_k)     # the lists store_recommendation would write
    hist, cos, _ = m.because(np.repeat(np.arange(U), top_k), ids.reshape(-1), 2, "both")
    want = io.StringIO()
    ranking.write_because(want, range(U), ids, vals, hist.reshape(U, top_k, 2), cos.reshape(U, top_k, 2))
    text = open(os.path.join(rdir, last[0])).read()
    assert text == want.getvalue() and len({tuple(l.split("\t")[:2]) for l in text.splitlines()}) == U * top_k
    for l in text.splitlines():
        u, i, _, rank, h, _ = l.split("\t")
        assert int(i) not in m.data.training_list[int(u)] and int(h) in m.data.training_list[int(u)] and int(rank) in (0, 1)
    e.close()
