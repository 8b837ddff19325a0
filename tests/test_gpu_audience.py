"""Audiences on the MI355X: bprx_audience_block against bprx_score_block / bprx_score_new_block (bit for bit where the header
promises bits) and the float64 restatement (tests/audience_ref.py), bprx_topk_rows_masked against the rules of tests/topk_ref.py,
the model methods on top of them and the files of train_rec --audience.

Allowance where bits are not promised (the rule of tests/test_gpu_new_items.py, _allow / _report): 32 x the max-abs deviation of
the FLOAT32 restatement from the float64 one over the case, never below one float32 ulp of the output's largest magnitude; every
comparison prints its triple.  Lists are never compared across precisions: a returned value is held against the float64 value
at the returned id and against the r-th largest float64 value of the masked row, and the list itself is checked exactly against
the GPU's own masked row (stable descending order; numpy_topk where the kernel flags the row), the method of
tests/test_gpu_similar.py."""
import gc
import io
import os

import numpy as np
import pytest
import torch

import audience_ref as A
import topk_ref as tr
from fashionvisualexpl_recommend_amd import _ffi, ranking, synth
from test_gpu_feat_explain import _bits, _snapshot, _tables, _unique_batches, _vbpr
from test_gpu_new_items import GUARD, PATTERN, _allow, _cli_dataset, _expected_lists, _model, _new_rows, _report
from test_gpu_similar import _bprmf

pytestmark = pytest.mark.gpu

D, NCOLS, N_NEW = 128, 100, 170                               # feature columns (real ones), rows from outside: one tile + 42
_REF = {}


def _case(U, I, k, d, dtype):
    """Tables, new rows and (r64, r32) of both score forms and of the BPRMF part, computed once per case and left unchanged."""
    key = (U, I, k, d, dtype)
    if key not in _REF:
        t = _tables(U, I, k, max(d, 1), D, NCOLS, dtype, seed=70 + k + d)
        Fn = _new_rows(N_NEW, D, NCOLS, dtype, seed=71)
        mf = {n: t[n] for n in ("Gu", "Gi", "Bi")}
        ref = {"mf": tuple(A.scores(mf, dtype, dt) for dt in (torch.float64, torch.float32))}
        if d:
            ref["cat"] = tuple(A.scores(t, dtype, dt) for dt in (torch.float64, torch.float32))
            ref["new"] = tuple(A.scores(t, dtype, dt, F=Fn) for dt in (torch.float64, torch.float32))
        _REF[key] = (t, Fn, ref)
    return _REF[key]


def _T(x):
    return np.ascontiguousarray(x.cpu().numpy().T)


# ---- bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("k,d", [(16, 12), (64, 64), (16, 0)])
@pytest.mark.parametrize("I", [300, 40])
@pytest.mark.parametrize("U", [300, 40])
def test_even_widths_have_the_bits_of_the_user_major_blocks(U, I, k, d, dtype):
    """Two full tiles + 44 and less than a tile on either side; even k and d: the transposed block, bit for bit."""
    t, Fn, _ = _case(U, I, k, d, dtype)
    m = _bprmf(t)                                              # BPRMF on the same Gu / Gi / Bi
    mf = m.audience_block(0, I).cpu().numpy()
    assert mf.shape == (I, U) and np.array_equal(_bits(mf), _bits(_T(m.score_block(0, U))))
    m.sync_check()
    m.close()
    if d == 0:
        return
    e = _vbpr(t, dtype)
    got = e.audience_block(0, I).cpu().numpy()
    assert got.shape == (I, U) and not np.isnan(got).any()
    assert np.array_equal(_bits(got), _bits(_T(e.score_block(0, U)))), "catalogue form"
    assert not np.array_equal(_bits(got), _bits(mf))          # (the visual part is there)
    P = e.project_rows(Fn)
    new = e.audience_block(0, N_NEW, P).cpu().numpy()
    assert new.shape == (N_NEW, U) and np.array_equal(_bits(new), _bits(_T(e.score_new_block(0, U, P)))), "Pq form"
    e.sync_check()
    e.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_a_factored_handle_after_adam_steps_has_the_same_bits(dtype):
    """GradFashion's handle (E_eff / Bp_eff composed by the library), lazy rows and P brought up to date by the gate itself."""
    from test_gpu_gradfashion import Dc, De, PAD, _engine as gf_engine, _setup as gf_setup
    U, I = 170, 300
    t, F = gf_setup(dtype, U=U, I=I)
    e = gf_engine(t, F, dtype, optimizer="adam_tf23", lr=2e-3, reg=1e-3, B=64)
    rs = np.random.RandomState(81)
    for _ in range(3):
        e.step(*(torch.as_tensor(rs.randint(m, size=64).astype(np.int32), device="cuda") for m in (U, I, I)))
    got = e.audience_block(0, I).cpu().numpy()                 # (the first read after the steps)
    assert np.array_equal(_bits(got), _bits(_T(e.score_block(0, U))))
    assert np.array_equal(_bits(got[127:129]), _bits(e.audience_block(127, 129).cpu().numpy()))
    P = e.project_rows(_new_rows(N_NEW, PAD[dtype], Dc + De, dtype, seed=82))
    assert np.array_equal(_bits(e.audience_block(0, N_NEW, P).cpu().numpy()), _bits(_T(e.score_new_block(0, U, P))))
    e.sync_check()
    e.close()


# ---- closeness where bits are not promised -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("k,d", [(7, 15), (17, 16), (7, 0)])
@pytest.mark.parametrize("U,I", [(300, 300), (40, 40), (300, 40)])
def test_odd_widths_are_close_to_the_float64_scores(U, I, k, d, dtype):
    """An odd k or d: bprx_score_block runs its non-MFMA kernel (another summation order), the audience entry pads K with zeros.
    Both restate the same float64 scores; the Pq form's counterpart is always on the MFMA path: bits for any d."""
    t, Fn, ref = _case(U, I, k, d, dtype)
    tag = "U=%d I=%d k=%d d=%d %s" % (U, I, k, d, dtype)
    if d == 0:
        m = _bprmf(t)
        gdev, allow = _report("audience bprmf " + tag, *ref["mf"], m.audience_block(0, I).cpu().numpy())
        sdev, _ = _report("score_block^T bprmf " + tag, *ref["mf"], _T(m.score_block(0, U)))
        assert gdev <= allow and sdev <= allow
        m.sync_check()
        m.close()
        return
    e = _vbpr(t, dtype)
    gdev, allow = _report("audience " + tag, *ref["cat"], e.audience_block(0, I).cpu().numpy())
    sdev, _ = _report("score_block^T " + tag, *ref["cat"], _T(e.score_block(0, U)))
    assert gdev <= allow and sdev <= allow
    P = e.project_rows(Fn)
    new = e.audience_block(0, N_NEW, P).cpu().numpy()
    ndev, nallow = _report("audience of new rows " + tag, *ref["new"], new)
    assert ndev <= nallow
    assert np.array_equal(_bits(new), _bits(_T(e.score_new_block(0, U, P))))
    e.sync_check()
    e.close()


# ---- ranges --------------------------------------------------------------------------------------------------------------------
RANGES = [(0, 1), (0, 127), (0, 128), (0, 129), (127, 129), (299, 300), (0, 300)]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_item_ranges_leave_a_rows_bits_alone(dtype):
    U, I = 170, 300
    t, _, _ = _case(U, I, 16, 12, dtype)
    e = _vbpr(t, dtype)
    m = _bprmf(t)
    P = e.project_rows(_new_rows(I, D, NCOLS, dtype, seed=72))
    for eng, Pq in ((e, None), (e, P), (m, None)):
        full = None
        for q0, q1 in RANGES[::-1]:                            # (the whole catalogue first)
            nq = q1 - q0
            for call in range(2):
                buf = torch.full((nq * U + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
                got = eng.audience_block(q0, q1, Pq, out=buf[:nq * U].view(nq, U)).cpu().numpy()
                assert (buf[nq * U:] == PATTERN).all(), "[%d,%d): wrote behind its output" % (q0, q1)
                full = got if full is None else full
                assert np.array_equal(_bits(got), _bits(full[q0:q1])), "[%d,%d) call %d" % (q0, q1, call)
        buf = torch.full((GUARD,), PATTERN, dtype=torch.float32, device="cuda")
        eng.audience_block(5, 5, Pq, out=buf)                  # q0 == q1: nothing is written
        assert (buf == PATTERN).all()
        eng.sync_check()
    e.close()
    m.close()


# ---- bprx_topk_rows_masked -----------------------------------------------------------------------------------------------------
def _masked_launch(e, width, K, seed=0):
    """gen_rows' rows at this width plus rows whose list masks everything; lists with ids outside [0, width) mixed in (ignored by
    the kernel, left out of what the checker masks).  Returns check_launch's failures."""
    fit = tuple(f for f in tr.FAMILIES if not (f[0] == "dup_train" and K > width < 2))         # (two train items need two columns)
    scores, train, fams = tr.gen_rows(width, K, fit, seed=seed)
    rs = np.random.RandomState(width + K)
    scores = np.concatenate([scores, scores[:6].copy()])
    train = train + [[] for _ in range(2)] + [rs.permutation(width).tolist() for _ in range(4)]
    fams = fams + ["no_list"] * 2 + ["whole_row"] * 4
    given = [l + [width, -3, width + 7, 2 ** 31 - 1] if r % 3 == 0 else list(l) for r, l in enumerate(train)]
    given[-1] = given[-1] + given[-1][:2]                     # a repeat, whatever the families drew
    assert any(len(l) == 0 for l in given) and any(len(l) != len(set(l)) for l in given)      # empty lists, repeats
    S = torch.as_tensor(scores, device="cuda").contiguous()
    idx, val, flag = (x.cpu().numpy() for x in e.topk_rows_masked(S, e.csr(given), K))
    bad = tr.check_launch(scores, train, fams, K, idx, val, flag, S.cpu().numpy())
    assert flag[-4:].all(), "a row masked as a whole came back unflagged"
    return bad, (scores, train, given, idx, val, flag)


@pytest.mark.parametrize("K", [1, 20, 1024])
@pytest.mark.parametrize("width", [1, 37, 256, 257, 1000])
def test_topk_rows_masked(width, K):
    from fashionvisualexpl_recommend_amd.engine import Engine
    t = _tables(20, 40, 16, 1, D, NCOLS, "fp32", seed=73)
    e = _bprmf(t)                                              # I = 40: the width is the call's, not the handle's
    bad, _ = _masked_launch(e, width, K)
    assert not bad, "%d rows: %s" % (len(bad), bad[:6])
    e.sync_check()
    e.close()
    if width == 1 and K == 1:                                  # an unbound handle may call it too (as bprx_topk_lists)
        u = Engine(model="bprmf", num_users=20, num_items=40, embed_k=16, optimizer="sgd", max_batch=64)
        bad, _ = _masked_launch(u, 37, 5)
        assert not bad
        u.close()


@pytest.mark.parametrize("K", [1, 20, 33])
def test_topk_rows_masked_at_catalogue_width_is_topk_lists(K):
    I = 40
    e = _bprmf(_tables(20, I, 16, 1, D, NCOLS, "fp32", seed=73))
    bad, (scores, train, given, idx, val, flag) = _masked_launch(e, I, K)
    assert not bad, bad[:6]
    S = torch.as_tensor(scores, device="cuda").contiguous()
    li, lv, lf = (x.cpu().numpy() for x in e.topk_lists(S, e.csr(given), K))
    assert np.array_equal(lf, flag)
    det = np.array([tr.classify(tr.mask(scores, train)[r], K, tr.n_unmasked(I, train[r])) == tr.DETERMINED for r in range(len(train))])
    assert det.any() and (flag[det] == 0).all()
    assert np.array_equal(idx[det], li[det]) and np.array_equal(_bits(val[det]), _bits(lv[det]))
    for bad_call in (lambda: e.topk_rows_masked(S, e.csr(given), 0), lambda: e.topk_rows_masked(S, e.csr(given), 1025)):
        with pytest.raises(_ffi.BprxError) as err:
            bad_call()
        assert err.value.code == _ffi.E_INVALID
    p = lambda x: x.data_ptr()
    ptr, items = e.csr(given)
    lib, n = e.lib, len(given)
    li, lv, lf = e._topk_out(n, 5)                                  # (device outputs for the raw calls)
    assert lib.bprx_topk_rows_masked(e.h, n, 0, p(S), p(ptr), p(items), 5, p(li), p(lv), p(lf), None) == _ffi.E_INVALID     # width < 1
    assert lib.bprx_topk_rows_masked(e.h, -1, I, p(S), p(ptr), p(items), 5, p(li), p(lv), p(lf), None) == _ffi.E_INVALID
    assert lib.bprx_topk_rows_masked(e.h, n, I, p(S), None, p(items), 5, p(li), p(lv), p(lf), None) == _ffi.E_INVALID
    assert lib.bprx_topk_rows_masked(e.h, n, I, None, p(ptr), p(items), 5, p(li), p(lv), p(lf), None) == _ffi.E_INVALID
    assert lib.bprx_topk_rows_masked(e.h, 0, I, None, None, None, 5, None, None, None, None) == 0                           # no rows
    e.sync_check()
    e.close()


# ---- lists ---------------------------------------------------------------------------------------------------------------------
ALMOST, NON_OWNERS = 11, [4, 77, 120]                         # item 11 is owned by all but three users


def _audience_model():
    """_model() (VBPR, bf16, U = 130, I = 60, k = 8, d = 20) with twin users 3 and 8 (equal scores for every item: lists numpy
    has to order) and an item nearly everybody owns."""
    from fashionvisualexpl_recommend_amd.models import VBPR
    m, raw = _model()
    Gu, Tu = (m.engine.t[n].cpu().numpy().copy() for n in ("Gu", "Tu"))
    m.engine.close()
    Gu[8], Tu[8] = Gu[3], Tu[3]
    Gu[100], Tu[100] = Gu[50], Tu[50]                         # (a second pair, with lists of their own)
    tl = [list(l) for l in m.data.training_list]
    for u in range(130):
        tl[u] = [i for i in tl[u] if i != ALMOST] + ([] if u in NON_OWNERS else [ALMOST])
    tl[3] = [i for i in tl[3] if i not in tl[8]] + tl[8]      # the twins own the same items: equal masked rows too
    tl[8] = list(tl[3])
    tl[20] = tl[20] + tl[20]                                  # a list that names its items twice
    m.data.training_list = tl
    return VBPR(m.data, m.params, init={"Gu": Gu, "Tu": Tu}, features=raw), raw


def _check_lists(tag, ids, vals, own, r64, r32, K):
    """ids / vals [n, kk] against the GPU's own MASKED rows `own` [n, U] and the float64 rows r64 (masked alike here)."""
    n, U = own.shape
    kk = ids.shape[1]
    _, _, wflag = _expected_lists(own, K)
    for r in range(n):
        want = own[r].argsort()[-K:][::-1][:kk] if wflag[r] else np.lexsort((np.arange(U), -own[r].astype(np.float64)))[:kk]
        wval = own[r][want]
        assert np.array_equal(ids[r], np.where(np.isneginf(wval), -1, want)) and np.array_equal(_bits(vals[r]), _bits(wval)), (tag, r)
    dev, allow = _allow(r64, r32)
    row64 = np.where(np.isneginf(own), -np.inf, r64)
    live = ids >= 0
    at = np.take_along_axis(row64, np.maximum(ids, 0), axis=1)
    rank = (-np.sort(-row64, axis=1))[:, :kk]
    assert np.isneginf(rank[~live]).all() and np.isneginf(vals[~live]).all()        # empty slots: where the masked row runs out
    at_id = float(np.abs(vals[live] - at[live]).max())
    by_rank = float(np.abs(vals[live] - rank[live]).max())
    print("%s: float32 deviation %.3e / allowance %.3e / GPU deviation at the id %.3e, by rank %.3e" % (tag, dev, allow, at_id, by_rank))
    assert at_id <= allow and by_rank <= allow
    return wflag


@pytest.mark.parametrize("block", [16, 1])
def test_model_audience(block):
    m, _ = _audience_model()
    e = m.engine
    U, I, K = 130, 60, 20
    m.evaluator.user_block = block                                 # four blocks of item rows / one row per block
    assert m.audience_k == 0
    owners = A.owners(m.data.training_list, I)
    assert [u for u in range(U) if u not in owners[ALMOST]] == NON_OWNERS
    assert [o.tolist() for o in ranking.owners_of(m.data.training_list, I)] == owners
    t = {n: e.t[n] for n in ("Gu", "Gi", "Bi", "Tu", "F", "E", "Bp")}
    r64, r32 = (A.scores(t, "bf16", dt) for dt in (torch.float64, torch.float32))
    raw_rows = e.audience_block(0, I).cpu().numpy()
    gdev, allow = _report("audience block of the model", r64, r32, raw_rows)
    assert gdev <= allow
    own = A.masked(raw_rows, owners)
    ids, vals = m.audience(k=K)
    assert ids.shape == vals.shape == (I, K) and ids.dtype == np.int64 and vals.dtype == np.float32
    wflag = _check_lists("audience block=%d" % block, ids, vals, own, r64, r32, K)
    assert 0 < wflag.sum() < I and wflag[ALMOST] == 1              # both kinds of row; no flagged row is skipped (all are checked)
    for i in range(I):
        assert not set(ids[i][ids[i] >= 0].tolist()) & set(owners[i]), "item %d lists an owner" % i
    assert sorted(ids[ALMOST, :3].tolist()) == NON_OWNERS and (ids[ALMOST, 3:] == -1).all()
    pick = [59, 0, ALMOST, 17, 17, 33]
    i2, v2 = m.audience(pick, k=K)
    assert np.array_equal(i2, ids[pick]) and np.array_equal(_bits(v2), _bits(vals[pick]))
    i3, v3 = m.audience(k=200)                                     # k > U: every non-owner, then -1
    assert i3.shape == (I, U)
    assert all(sorted(i3[i][i3[i] >= 0].tolist()) == [u for u in range(U) if u not in owners[i]] for i in range(I))
    assert int((ids[ALMOST] >= 0).sum()) == 3                      # three entries
    e.sync_check()
    e.close()


def test_model_audience_new():
    m, raw = _audience_model()
    e = m.engine
    U, K, n = 130, 20, 33
    new_raw = np.concatenate([raw[[5, 9]], synth.make_features(n - 2, 128, seed=74) * 5.0])
    Fd = m.prepare_new_items(new_raw)
    t = {nm: e.t[nm] for nm in ("Gu", "Gi", "Bi", "Tu", "F", "E", "Bp")}
    r64, r32 = (A.scores(t, "bf16", dt, F=Fd.float()) for dt in (torch.float64, torch.float32))
    own = e.audience_block(0, n, e.project_rows(Fd)).cpu().numpy()
    gdev, allow = _report("audience_new block", r64, r32, own)
    assert gdev <= allow
    for block in (16, 1):
        m.evaluator.user_block = block
        ids, vals = m.audience_new(new_raw, k=K)
        assert ids.shape == vals.shape == (n, K) and (ids >= 0).all()      # nothing is masked
        wflag = _check_lists("audience_new block=%d" % block, ids, vals, own, r64, r32, K)
        assert wflag.any()                                             # the twin users
        i2, v2 = m.audience_new(Fd, k=K)                               # a prepared table: the same lists
        assert np.array_equal(i2, ids) and np.array_equal(_bits(v2), _bits(vals))
    assert m.audience_new(new_raw, k=200)[0].shape == (n, U)
    e.sync_check()
    e.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------
def _all_calls(e, F, own):
    P = e.project_rows(F)
    blk = e.audience_block(3, 211)
    return [blk, e.audience_block(0, int(P.shape[0]), P), e.topk_rows_masked(blk, own, 20)]


@pytest.mark.parametrize("opt,form", [("sgd", None), ("adam_tf23", "lazy"), ("adam_tf23", "sweep")])
def test_the_calls_leave_the_state_alone(monkeypatch, opt, form):
    """Tables and Adam slots are bit-identical before and after the calls, and a 6-step run with them between steps 3 and 4 ends
    bit-identical to a run without them (duplicate-free batches: the step itself is then free of atomic-order noise)."""
    t = _tables(300, 300, 16, 12, D, NCOLS, "bf16", seed=17)
    batches = _unique_batches(300, 300, 64, 6, seed=18)
    F = _new_rows(77, D, NCOLS, "bf16", seed=75)
    rs = np.random.RandomState(76)
    lists = [rs.choice(300, rs.randint(0, 9), replace=False).tolist() for _ in range(208)]
    lib = _ffi.lib()
    end = []
    if form is not None:
        monkeypatch.setenv("BPRX_ADAM_LAZY", "1" if form == "lazy" else "0")
    for with_calls in (False, True):
        e = _vbpr(t, "bf16", optimizer=opt, B=64)
        own = e.csr(lists)
        if form is not None:
            assert e.adam_is_lazy() == (form == "lazy")
        for s, b in enumerate(batches):
            if s == 3 and with_calls:
                e.sync_adam()
                before = _snapshot(e)
                held = lib.bprx_live_device_allocs()
                _all_calls(e, F, own)
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


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable_and_no_allocation_behind():
    import test_gpu_acf as ga
    import attentive_ref as ar
    import test_gpu_attentive as gat
    from acf_ref import random_tables
    from fashionvisualexpl_recommend_amd.engine import Engine
    lib = _ffi.lib()
    gc.collect()
    live = lib.bprx_live_device_allocs()
    U, I = 50, 80
    t = _tables(U, I, 16, 12, 256, 200, "bf16", seed=77)
    e, f8, m = _vbpr(t, "bf16"), _vbpr(t, "fp8"), _bprmf(t)
    unbound = Engine(model="vbpr", num_users=U, num_items=I, embed_k=16, embed_d=12, feat_dim=256, feat_dtype="bf16", optimizer="sgd",
                     max_batch=64)
    rs = np.random.RandomState(78)
    acf = ga._engine(random_tables(rs, 12, I, 16, 128, 64, 64, scale=10.0), ga._features(rs, I, 9, 128, "fp32"),
                     ga._lists(rs, 12, I, rs.randint(0, 15, 12)))
    P = e.project_rows(_new_rows(40, 256, 200, "bf16", seed=79))
    held = lib.bprx_live_device_allocs()
    good = e.audience_block(0, I).cpu().numpy()
    good_new = e.audience_block(0, 40, P).cpu().numpy()
    out = torch.full((I * U + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    assert lib.bprx_live_device_allocs() == held                    # the calls allocated nothing

    def usable():
        assert np.array_equal(_bits(good), _bits(e.audience_block(0, I).cpu().numpy()))
        assert np.array_equal(_bits(good_new), _bits(e.audience_block(0, 40, P).cpu().numpy()))
        e.sync_check()

    p = lambda x: None if x is None else x.data_ptr()
    block = lambda h, Pq, nq, q0, q1, o: lib.bprx_audience_block(h, p(Pq), nq, q0, q1, p(o), None)
    assert block(None, None, I, 0, 1, out) == _ffi.E_INVALID
    bad = [lambda: block(e.h, None, I, 0, 1, None), lambda: block(e.h, P, 40, 0, 1, None),          # null pointer
           lambda: block(e.h, None, I - 1, 0, 1, out), lambda: block(e.h, None, I + 1, 0, 1, out),  # the catalogue: nq == num_items
           lambda: block(e.h, None, 0, 0, 0, out),
           lambda: block(e.h, None, I, -1, 1, out), lambda: block(e.h, None, I, 2, 1, out),         # ranges
           lambda: block(e.h, None, I, 0, I + 1, out), lambda: block(e.h, P, 40, 0, 41, out),
           lambda: block(e.h, P, -1, 0, 0, out), lambda: block(e.h, P, 1 << 31, 0, 1, out),
           lambda: block(e.h, P, (1 << 31) - 1, 0, 65535 * 128 + 1, out)]                           # more than 65535 row tiles
    for q, call in enumerate(bad):
        assert call() == _ffi.E_INVALID, q
        assert lib.bprx_last_error(e.h).decode().startswith("audience_block"), q
    usable()
    assert (out == PATTERN).all()                                   # no rejected call wrote anything
    assert block(e.h, None, I, 7, 7, out) == 0 and block(e.h, P, 40, 40, 40, out) == 0 and block(m.h, None, I, I, I, out) == 0
    torch.cuda.synchronize()
    assert (out == PATTERN).all()                                   # q0 == q1: BPRX_OK, nothing is written
    # handles of the wrong kind, unbound tables
    for eng, calls, code in ((m, [lambda: m.audience_block(0, 1, P)], _ffi.E_INVALID),              # Pq with a BPRMF handle
                             (f8, [lambda: f8.audience_block(0, 1, P)], _ffi.E_INVALID),            # Pq with an fp8 handle
                             (acf, [lambda: acf.audience_block(0, 1), lambda: acf.audience_block(0, 1, P)], _ffi.E_INVALID),
                             (unbound, [lambda: unbound.audience_block(0, 1), lambda: unbound.audience_block(0, 1, P)], _ffi.E_STATE)):
        for call in calls:
            with pytest.raises(_ffi.BprxError) as err:
                call()
            assert err.value.code == code, (eng, code)
    assert "fp8" in lib.bprx_last_error(f8.h).decode()
    ars = np.random.RandomState(80)                                 # an AttentiveFashion handle (U = 5, I = 8)
    af = gat._engine(ar.random_tables(ars, 5, 8, 16, 37, 11, 64, bias=True), ar.random_inputs(ars, 8, 37, 11))
    with pytest.raises(_ffi.BprxError) as err:
        af.audience_block(0, 1)
    assert err.value.code == _ffi.E_INVALID and af.score_block(0, 5).shape == (5, 8)
    af.close()
    # every handle goes on working: the fp8 handle's catalogue form is its own score block, transposed
    assert np.array_equal(_bits(f8.audience_block(0, I).cpu().numpy()), _bits(_T(f8.score_block(0, U))))
    assert np.array_equal(_bits(m.audience_block(0, I).cpu().numpy()), _bits(_T(m.score_block(0, U))))
    assert acf.score_block(0, 12).shape == (12, I)
    usable()
    assert lib.bprx_live_device_allocs() == held
    for eng in (e, f8, m, unbound, acf):
        eng.close()
    assert lib.bprx_live_device_allocs() == live


# ---- files ---------------------------------------------------------------------------------------------------------------------
def _file_of(ids, vals, labels):
    out = io.StringIO()
    for r, lab in enumerate(labels):
        n = int((ids[r] >= 0).sum())
        ranking.write_ranked(out, [lab], ids[r:r + 1, :n], vals[r:r + 1, :n])
    return out.getvalue().encode()


@pytest.mark.parametrize("rec,dtype", [("vbpr", "bf16"), ("bprmf", "fp32")])
def test_cli_writes_audience_files_next_to_unchanged_recommendations(tmp_path, rec, dtype):
    from fashionvisualexpl_recommend_amd import train_rec
    paths, n_new, _ = _cli_dataset(tmp_path, "vbpr")
    U, I, K = 30, 60, 5
    common = ["--rec", rec, "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--reg", "0.01", "--top_k", "10", "--lr", "0.01", "--dtype", dtype]
    new = (["--new_items"] + paths) if rec == "vbpr" else []
    res = [str(tmp_path / ("res%d" % q)) for q in range(3)]
    train_rec.train(common + ["--results_root", res[0]] + new)
    (tmp_path / "ids.txt").write_text("41\n7\n\n41\n0\n")
    train_rec.train(common + ["--results_root", res[2], "--audience", str(K), "--audience_items", str(tmp_path / "ids.txt")] + new)
    picked = train_rec._last_model
    pick_ids, pick_vals = picked.audience([41, 7, 41, 0])
    picked.engine.close()
    train_rec.train(common + ["--results_root", res[1], "--audience", str(K)] + new)
    m = train_rec._last_model
    rdir = [os.path.join(r, "rec_results", "toy", rec) for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] if "audience-" in f]
    assert [f for f in files[1] if "audience-" not in f] == files[0] == [f for f in files[2] if "audience-" not in f]
    base = [f for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(base) == 2
    last = [f for f in base if f.startswith("recs-")][0]
    owners = A.owners(m.data.training_list, I)
    ids, vals = m.audience()
    assert ids.shape == (I, K)
    for f in base:
        for g in [f] + ([f.replace("recs-", "new-recs-", 1)] if new else []):      # the bytes of the run without the flag
            assert open(os.path.join(rdir[0], g), "rb").read() == open(os.path.join(rdir[1], g), "rb").read(), g
        a, na = f.replace("recs-", "audience-", 1), f.replace("recs-", "new-audience-", 1)
        assert a in files[1] and a in files[2] and (na in files[1]) == bool(new) and (na in files[2]) == bool(new)
        rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], a))]
        assert all(len(r) == 3 for r in rows) and [int(r[0]) for r in rows] == sorted(int(r[0]) for r in rows)
        for i in range(I):
            blk = [r for r in rows if int(r[0]) == i]
            sc = [float(r[2]) for r in blk]
            assert len(blk) == min(K, U - len(owners[i])) and sc == sorted(sc, reverse=True)
            assert not {int(r[1]) for r in blk} & set(owners[i]) and all(0 <= int(r[1]) < U for r in blk)
    # the files of the last epoch are the model's lists as it stands now, formatted by write_ranked
    a = os.path.join(rdir[1], last.replace("recs-", "audience-", 1))
    assert open(a, "rb").read() == _file_of(ids, vals, range(I))
    assert open(os.path.join(rdir[2], last.replace("recs-", "audience-", 1)), "rb").read() == _file_of(pick_ids, pick_vals, [41, 7, 41, 0])
    if new:
        nid, nval = m.audience_new(np.load(paths[0]))
        assert nid.shape == (n_new, K)
        na = os.path.join(rdir[1], last.replace("recs-", "new-audience-", 1))
        assert open(na, "rb").read() == _file_of(nid, nval, range(n_new))
    # no byte depends on the evaluator's block of rows
    for block in (16, 1):
        m.evaluator.user_block = block
        m.evaluator.store_audience(str(tmp_path / "again.tsv"))
        assert open(str(tmp_path / "again.tsv"), "rb").read() == open(a, "rb").read(), block
        if new:
            m.evaluator.store_audience_new(str(tmp_path / "again_new.tsv"), np.load(paths[0]))
            assert open(str(tmp_path / "again_new.tsv"), "rb").read() == open(na, "rb").read(), block
    assert any(f.startswith("best-audience-") for f in files[1])
    assert not new or any(f.startswith("best-new-audience-") for f in files[1])
    m.engine.sync_check()
    m.engine.close()
