"""Similar items on the MI355X: bprx_sim_rnorm / bprx_sim_block against the float64 restatement (tests/similar_ref.py), the model
methods on top of them and the files of train_rec --similar_items.

Allowance per compared output (the rule of tests/test_gpu_feat_explain.py / test_gpu_new_items.py): 32 x the max-abs deviation of
the FLOAT32 restatement from the float64 one over the case, never below one float32 ulp of the output's largest magnitude.  Every
comparison prints its triple (float32 deviation / allowance / GPU deviation).  What is exact is checked exactly: a row's bits
whatever the query range and the call, s(i, j) against s(j, i), twins, the zero row, the buffer behind an output, the state.

Near-ties do occur inside a top-20 (gaps down to 1e-8), so list identities are never compared across precisions: a returned value
is held against the float64 value at the returned id and against the r-th largest float64 value of the row, and the list itself
is checked exactly against the GPU's own masked row (stable descending order; numpy_topk where the kernel flags the row)."""
import gc
import os

import numpy as np
import pytest
import torch

import similar_ref as S
from fashionvisualexpl_recommend_amd import _ffi, ranking, synth
from test_gpu_feat_explain import _bits, _snapshot, _tables, _unique_batches, _vbpr
from test_gpu_new_items import GUARD, PATTERN, _allow, _cli_dataset, _expected_lists, _model, _new_rows, _report

pytestmark = pytest.mark.gpu

FEAT_D = {"fp32": 400, "bf16": 512}                            # 390 real columns, zero padding behind them
_REF = {}


def _bprmf(t):
    from fashionvisualexpl_recommend_amd.engine import Engine
    U, k = t["Gu"].shape
    e = Engine(model="bprmf", num_users=U, num_items=t["Gi"].shape[0], embed_k=k, optimizer="sgd", lr=0.05, reg=0.0, max_batch=64)
    return e.bind(t["Gu"], t["Gi"], t["Bi"])


def _case(I, k, d, dtype, special=False):
    """Tables and, per space, (r64, r32): the cosines of the catalogue in float64 and float32.  Computed once per case and left
    unchanged.  special: items 7 and 19 are twins (bit-equal Gi and feature rows), item 5 is a zero row in every space."""
    key = (I, k, d, dtype, special)
    if key not in _REF:
        t = _tables(20, I, k, d, FEAT_D[dtype], 390, dtype, seed=60 + k + d)
        if special:
            t["Gi"][19], t["F"][19] = t["Gi"][7], t["F"][7]
            t["Gi"][5], t["F"][5] = 0, 0
        ref = {sp: tuple(S.cosine(S.item_vectors(t, sp, dtype, dt), dt) for dt in (torch.float64, torch.float32)) for sp in S.SPACES}
        _REF[key] = (t, ref)
    return _REF[key]


def _whole(e, space):
    rn = e.sim_rnorm(space)
    return rn, e.sim_block(space, 0, e.I, rn).cpu().numpy()


# ---- shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("k,d", [(16, 12), (7, 15), (17, 16), (64, 64)])
@pytest.mark.parametrize("I", [300, 40])
def test_shapes_spaces_and_symmetry(I, k, d, dtype):
    """Two full column tiles + 44 and less than a tile; widths below, at and above the 16-column K chunk, odd ones included."""
    t, ref = _case(I, k, d, dtype)
    e = _vbpr(t, dtype)
    for space in S.SPACES:
        r64, r32 = ref[space]
        rn, out = _whole(e, space)
        z64, z32 = (S.item_vectors(t, space, dtype, dt) for dt in (torch.float64, torch.float32))
        g_rn, a_rn = _report("rnorm I=%d k=%d d=%d %s %s" % (I, k, d, dtype, space), S.rnorm(z64), S.rnorm(z32, torch.float32),
                             rn.cpu().numpy())
        gdev, allow = _report("cosine I=%d k=%d d=%d %s %s" % (I, k, d, dtype, space), r64, r32, out)
        assert g_rn <= a_rn and gdev <= allow
        assert out.shape == (I, I) and not np.isnan(out).any()
        assert np.array_equal(_bits(out), _bits(out.T.copy())), "%s: s(i, j) != s(j, i)" % space
    m = _bprmf(t)                                              # a BPRMF handle: the same Gi, the same kernel, the same bits
    assert np.array_equal(_bits(_whole(m, "latent")[1]), _bits(_whole(e, "latent")[1]))
    for eng in (e, m):
        eng.sync_check()
        eng.close()


# ---- query ranges --------------------------------------------------------------------------------------------------------------
RANGES = [(0, 1), (0, 127), (0, 128), (0, 129), (127, 129), (299, 300), (0, 300)]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_query_ranges_leave_a_rows_bits_alone(dtype):
    I = 300
    t, _ = _case(I, 16, 12, dtype)
    e = _vbpr(t, dtype)
    P = e.project_rows(_new_rows(I, FEAT_D[dtype], 390, dtype, seed=61))
    forms = [(sp, None, None) for sp in S.SPACES] + [("visual", P, e.sim_rnorm("visual", P))]
    for space, Pq, rq in forms:
        rn = e.sim_rnorm(space)
        assert np.array_equal(_bits(rn.cpu().numpy()), _bits(e.sim_rnorm(space).cpu().numpy()))
        full = None
        for q0, q1 in RANGES[::-1]:                            # (the whole catalogue first)
            nq = q1 - q0
            for call in range(2):
                buf = torch.full((nq * I + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
                got = e.sim_block(space, q0, q1, rn, Pq, rq, out=buf[:nq * I].view(nq, I)).cpu().numpy()
                assert (buf[nq * I:] == PATTERN).all(), "%s [%d,%d): wrote behind its output" % (space, q0, q1)
                full = got if full is None else full
                assert np.array_equal(_bits(got), _bits(full[q0:q1])), "%s [%d,%d) call %d" % (space, q0, q1, call)
        buf = torch.full((GUARD,), PATTERN, dtype=torch.float32, device="cuda")
        e.sim_block(space, 5, 5, rn, Pq, rq, out=buf)          # q0 == q1: nothing is written
        assert (buf == PATTERN).all()
    e.sync_check()
    e.close()


# ---- twins and the zero row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_twins_and_the_zero_row(dtype):
    I = 300
    t, ref = _case(I, 16, 12, dtype, special=True)
    e = _vbpr(t, dtype)
    own = e.csr([[q] for q in range(I)])
    for space in S.SPACES:
        r64, r32 = ref[space]
        rn, out = _whole(e, space)
        gdev, allow = _report("twins %s %s" % (dtype, space), r64, r32, out)
        assert gdev <= allow
        assert np.array_equal(_bits(out[7]), _bits(out[19])) and abs(float(out[7, 19]) - 1.0) <= allow
        assert float(rn[5]) == 0.0 and (out[5] == 0.0).all() and (out[:, 5] == 0.0).all() and not np.isnan(out).any()
        assert np.array_equal(_bits(out), _bits(out.T.copy()))
        idx, val, flag = (x.cpu().numpy() for x in e.topk_lists(torch.as_tensor(out, device="cuda"), own, 5))
        assert idx[7, 0] == 19 and idx[19, 0] == 7 and flag[5] == 1
    e.sync_check()
    e.close()


# ---- one scale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_rows_from_outside_sit_on_the_catalogues_scale(dtype):
    """The catalogue's own feature rows as Pq: both forms restate the same float64 values (no bit equality: the tiled projection
    of the catalogue sums in another order)."""
    I = 300
    t, ref = _case(I, 16, 12, dtype)
    e = _vbpr(t, dtype)
    r64, r32 = ref["visual"]
    rn, cat = _whole(e, "visual")
    P = e.project_rows(t["F"])
    rq = e.sim_rnorm("visual", P)
    new = e.sim_block("visual", 0, I, rn, P, rq).cpu().numpy()
    g_new, allow = _report("one scale %s rows" % dtype, r64, r32, new)
    g_cat, _ = _report("one scale %s catalogue" % dtype, r64, r32, cat)
    z64, z32 = (S.item_vectors(t, "visual", dtype, dt) for dt in (torch.float64, torch.float32))
    g_rq, a_rq = _report("one scale %s rnorm of rows" % dtype, S.rnorm(z64), S.rnorm(z32, torch.float32), rq.cpu().numpy())
    assert g_new <= allow and g_cat <= allow and g_rq <= a_rq
    e.sync_check()
    e.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------
def _all_calls(e, F):
    P = e.project_rows(F)
    outs = []
    for space in S.SPACES:
        rn = e.sim_rnorm(space)
        outs += [rn, e.sim_block(space, 3, 211, rn)]
    rq = e.sim_rnorm("visual", P)
    return outs + [rq, e.sim_block("visual", 0, int(P.shape[0]), outs[2], P, rq)]


@pytest.mark.parametrize("opt,form", [("sgd", None), ("adam_tf23", "lazy"), ("adam_tf23", "sweep")])
def test_the_calls_leave_the_state_alone(monkeypatch, opt, form):
    """Tables and Adam slots are bit-identical before and after the calls, and a 6-step run with them between steps 3 and 4 ends
    bit-identical to a run without them (duplicate-free batches: the step itself is then free of atomic-order noise)."""
    t = _tables(300, 600, 16, 12, 128, 100, "bf16", seed=17)
    batches = _unique_batches(300, 600, 64, 6, seed=18)
    F = _new_rows(77, 128, 100, "bf16", seed=62)
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
                held = lib.bprx_live_device_allocs()
                _all_calls(e, F)
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


@pytest.mark.parametrize("first", ["sim_rnorm", "sim_block"])
def test_a_pending_dense_update_is_settled_first(monkeypatch, first):
    """Right after a step that was not asked for its loss (its E|Bp update is still pending): the calls see the tables of a handle
    that never defers."""
    import test_gpu_dense_defer as dd
    ea, eb = dd._pair(monkeypatch, 256, 20, "bf16", "sgd")
    for s in range(2):
        b = dd._batch(300 + s)
        ea.step(*b, want_loss=False); eb.step(*b, want_loss=False)
    assert ea.dense_pending() and not eb.dense_pending()
    rn_b = eb.sim_rnorm("both")
    if first == "sim_rnorm":
        rn_a = ea.sim_rnorm("both")
    else:                                                      # (sim_block itself meets the pending update)
        got = ea.sim_block("both", 0, 129, rn_b)
        assert not ea.dense_pending()
        assert torch.equal(got, eb.sim_block("both", 0, 129, rn_b))
        rn_a = ea.sim_rnorm("both")
    assert not ea.dense_pending()
    assert torch.equal(rn_a, rn_b) and torch.equal(ea.sim_block("both", 0, 129, rn_a), eb.sim_block("both", 0, 129, rn_b))
    dd._same_tables(ea, eb, "after the calls")
    dd._close(ea, eb)


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable_and_no_allocation_behind():
    import test_gpu_acf as ga
    from acf_ref import random_tables
    from fashionvisualexpl_recommend_amd.engine import Engine
    lib = _ffi.lib()
    gc.collect()
    live = lib.bprx_live_device_allocs()
    I = 80
    t = _tables(50, I, 16, 12, 256, 200, "bf16", seed=63)
    e, f8, m = _vbpr(t, "bf16"), _vbpr(t, "fp8"), _bprmf(t)
    unbound = Engine(model="vbpr", num_users=50, num_items=I, embed_k=16, embed_d=12, feat_dim=256, feat_dtype="bf16", optimizer="sgd",
                     max_batch=64)
    rs = np.random.RandomState(64)
    acf = ga._engine(random_tables(rs, 12, I, 16, 128, 64, 64, scale=10.0), ga._features(rs, I, 9, 128, "fp32"),
                     ga._lists(rs, 12, I, rs.randint(0, 15, 12)))
    P = e.project_rows(_new_rows(40, 256, 200, "bf16", seed=65))
    held = lib.bprx_live_device_allocs()
    rn, good = _whole(e, "both")
    rv = e.sim_rnorm("visual")
    rq = e.sim_rnorm("visual", P)
    good_new = e.sim_block("visual", 0, 40, rv, P, rq).cpu().numpy()
    out = torch.full((I * I + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    assert lib.bprx_live_device_allocs() == held                    # the calls allocated nothing

    def usable():
        assert np.array_equal(_bits(good), _bits(_whole(e, "both")[1]))
        assert np.array_equal(_bits(good_new), _bits(e.sim_block("visual", 0, 40, rv, P, rq).cpu().numpy()))
        e.sync_check()

    p = lambda x: None if x is None else x.data_ptr()
    norm = lambda h, space, Pq, nq, r: lib.bprx_sim_rnorm(h, space, p(Pq), nq, p(r), None)
    block = lambda h, space, Pq, nq, q0, q1, a, b, o: lib.bprx_sim_block(h, space, p(Pq), nq, q0, q1, p(a), p(b), p(o), None)
    assert norm(None, 0, None, I, rn) == _ffi.E_INVALID and block(None, 0, None, I, 0, 1, rn, rn, out) == _ffi.E_INVALID
    bad = [lambda: norm(e.h, 1, None, I, None),                                            # null pointers
           lambda: block(e.h, 1, None, I, 0, 1, None, rv, out), lambda: block(e.h, 1, None, I, 0, 1, rv, None, out),
           lambda: block(e.h, 1, None, I, 0, 1, rv, rv, None),
           lambda: norm(e.h, 3, None, I, rn), lambda: norm(e.h, -1, None, I, rn),         # unknown spaces
           lambda: block(e.h, 3, None, I, 0, 1, rn, rn, out),
           lambda: norm(e.h, 0, P, 40, rq), lambda: norm(e.h, 2, P, 40, rq),              # rows from outside: visual only
           lambda: block(e.h, 0, P, 40, 0, 40, rq, rn, out), lambda: block(e.h, 2, P, 40, 0, 40, rq, rn, out),
           lambda: norm(e.h, 1, None, I - 1, rn), lambda: norm(e.h, 1, None, I + 1, rn),  # the catalogue: nq == num_items
           lambda: block(e.h, 1, None, I + 1, 0, 1, rv, rv, out),
           lambda: norm(e.h, 1, P, -1, rq), lambda: norm(e.h, 1, P, 1 << 31, rq),         # ranges
           lambda: block(e.h, 1, None, I, -1, 1, rv, rv, out), lambda: block(e.h, 1, None, I, 2, 1, rv, rv, out),
           lambda: block(e.h, 1, None, I, 0, I + 1, rv, rv, out), lambda: block(e.h, 1, P, 40, 0, 41, rq, rv, out),
           lambda: block(e.h, 1, P, 1 << 31, 0, 1, rq, rv, out)]
    for q, call in enumerate(bad):
        assert call() == _ffi.E_INVALID, q
        assert lib.bprx_last_error(e.h).decode().startswith("sim_"), q
    usable()
    assert (out == PATTERN).all()                                   # no rejected call wrote anything
    assert block(e.h, 1, None, I, 7, 7, rv, rv, out) == 0 and block(e.h, 1, P, 40, 40, 40, rq, rv, out) == 0
    assert norm(e.h, 1, P, 0, rq) == 0
    torch.cuda.synchronize()
    assert (out == PATTERN).all()                                   # q0 == q1, nq == 0: BPRX_OK, nothing is written
    # handles of the wrong kind, fp8 in a space that reads P, unbound tables
    for eng, spaces, code in ((m, ("visual", "both"), _ffi.E_INVALID), (f8, ("visual", "both"), _ffi.E_INVALID),
                              (acf, S.SPACES, _ffi.E_INVALID), (unbound, S.SPACES, _ffi.E_STATE)):
        for space in spaces:
            for call in (lambda: eng.sim_rnorm(space), lambda: eng.sim_block(space, 0, 1, rn)):
                with pytest.raises(_ffi.BprxError) as err:
                    call()
                assert err.value.code == code, (space, code)
    msg = lib.bprx_last_error(f8.h).decode()
    assert "fp8" in msg and "new items" not in msg
    with pytest.raises(ValueError):
        e.sim_block("visual", 0, 40, rv, P)                         # rows from outside come with their norms
    # every handle goes on working: fp8 and BPRMF in the latent space give the bits of the bf16 handle (the same Gi)
    lat = _whole(e, "latent")[1]
    assert np.array_equal(_bits(_whole(f8, "latent")[1]), _bits(lat)) and np.array_equal(_bits(_whole(m, "latent")[1]), _bits(lat))
    assert f8.score_block(0, 50).shape == (50, I) and acf.score_block(0, 12).shape == (12, I)
    usable()
    assert lib.bprx_live_device_allocs() == held
    for eng in (e, f8, m, unbound, acf):
        eng.close()
    assert lib.bprx_live_device_allocs() == live


# ---- lists ---------------------------------------------------------------------------------------------------------------------
def _check_lists(tag, ids, vals, own, r64, r32, K, masked):
    """ids / vals [n, kk] against the GPU's own rows `own` [n, I] (already masked where `masked`) and the float64 rows r64."""
    n, I = own.shape
    kk = ids.shape[1]
    _, _, wflag = _expected_lists(own, K)
    for r in range(n):
        want = own[r].argsort()[-K:][::-1][:kk] if wflag[r] else np.lexsort((np.arange(I), -own[r].astype(np.float64)))[:kk]
        assert np.array_equal(ids[r], want) and np.array_equal(_bits(vals[r]), _bits(own[r][want])), (tag, r)
    dev, allow = _allow(r64, r32)
    row64 = np.where(np.isneginf(own), -np.inf, r64) if masked else r64
    at_id = float(np.abs(vals - np.take_along_axis(row64, ids, axis=1)).max())
    by_rank = float(np.abs(vals - (-np.sort(-row64, axis=1))[:, :kk]).max())
    print("%s: float32 deviation %.3e / allowance %.3e / GPU deviation at the id %.3e, by rank %.3e" % (tag, dev, allow, at_id, by_rank))
    assert at_id <= allow and by_rank <= allow
    return wflag


@pytest.mark.parametrize("space", [None, "latent", "both"])
def test_model_similar_items(space):
    from fashionvisualexpl_recommend_amd.models import VBPR
    m, raw = _model()                                              # VBPR, bf16, I = 60, k = 8, d = 20
    I, K = 60, 20
    Gi = m.engine.t["Gi"].cpu().numpy().copy()
    m.engine.close()
    Gi[19], raw[19] = Gi[7], raw[7]                                # twins: rows with equal cosines, lists numpy has to order
    m = VBPR(m.data, m.params, init={"Gi": Gi}, features=raw)
    e = m.engine
    m.evaluator.user_block = 16                                    # four blocks of item rows
    name = "visual" if space is None else space
    assert m.similar_space == "visual" and m.similar_k == 0
    t = {n: e.t[n] for n in ("Gi", "F", "E", "Bp")}
    r64, r32 = (S.cosine(S.item_vectors(t, name, "bf16", dt), dt) for dt in (torch.float64, torch.float32))
    own = _whole(e, name)[1]
    own[np.arange(I), np.arange(I)] = -np.inf
    ids, vals = m.similar_items(k=K, space=space)
    assert ids.shape == vals.shape == (I, K) and ids.dtype == np.int64 and vals.dtype == np.float32
    assert not (ids == np.arange(I)[:, None]).any() and ids[7, 0] == 19 and ids[19, 0] == 7
    wflag = _check_lists("similar_items %s" % name, ids, vals, own, r64, r32, K, masked=True)
    assert 0 < wflag.sum() < I                                     # both kinds of row
    pick = [59, 0, 17, 17, 33]
    i2, v2 = m.similar_items(pick, k=K, space=space)
    assert np.array_equal(i2, ids[pick]) and np.array_equal(_bits(v2), _bits(vals[pick]))
    i3, v3 = m.similar_items(k=100, space=space)                   # k >= I: every other item, the item itself never
    assert i3.shape == (I, I - 1) and all(sorted(i3[r].tolist()) == [j for j in range(I) if j != r] for r in range(I))
    assert np.isfinite(v3).all()
    e.sync_check()
    e.close()


def test_model_similar_to_new():
    m, raw = _model()
    I, K, n = 60, 20, 33
    e = m.engine
    new_raw = np.concatenate([raw[[5, 9]], synth.make_features(n - 2, 128, seed=66) * 5.0])
    Fd = m.prepare_new_items(new_raw)
    t = {nm: e.t[nm] for nm in ("Gi", "F", "E", "Bp")}
    z = {dt: (S.item_vectors(t, "visual", "bf16", dt), S.item_vectors(t, "visual", "bf16", dt, F=Fd)) for dt in (torch.float64, torch.float32)}
    r64, r32 = (S.cosine(z[dt][0], dt, zq=z[dt][1]) for dt in (torch.float64, torch.float32))
    P = e.project_rows(Fd)
    rn, rq = e.sim_rnorm("visual"), e.sim_rnorm("visual", P)
    own = e.sim_block("visual", 0, n, rn, P, rq).cpu().numpy()
    gdev, allow = _report("similar_to_new block", r64, r32, own)
    assert gdev <= allow
    ids, vals = m.similar_to_new(new_raw, k=K)
    assert ids.shape == vals.shape == (n, K)
    _check_lists("similar_to_new", ids, vals, own, r64, r32, K, masked=False)
    assert ids[0, 0] == 5 and ids[1, 0] == 9 and abs(float(vals[0, 0]) - 1.0) <= allow      # a catalogue row finds itself
    i2, v2 = m.similar_to_new(Fd, k=K)                             # a prepared table: the same lists
    assert np.array_equal(i2, ids) and np.array_equal(_bits(v2), _bits(vals))
    assert m.similar_to_new(new_raw, k=100)[0].shape == (n, I)
    e.sync_check()
    e.close()


# ---- files ---------------------------------------------------------------------------------------------------------------------
def _rows(path):
    return [l.rstrip("\n").split("\t") for l in open(path)]


def _well_formed(rows, n_rows, kk, width, no_self):
    assert len(rows) == n_rows * kk and all(len(r) == 3 for r in rows)
    assert [int(r[0]) for r in rows] == [q for q in range(n_rows) for _ in range(kk)]
    assert all(0 <= int(r[1]) < width for r in rows) and all(-1.0001 <= float(r[2]) <= 1.0001 for r in rows)
    for q in range(n_rows):
        blk = rows[q * kk:(q + 1) * kk]
        sc = [float(r[2]) for r in blk]
        assert sc == sorted(sc, reverse=True) and len({r[1] for r in blk}) == kk
        assert not no_self or str(q) not in {r[1] for r in blk}


@pytest.mark.parametrize("rec,dtype,space", [("vbpr", "bf16", None), ("grad_fashion", "fp32", "both"), ("bprmf", "fp32", None)])
def test_cli_writes_sim_files_next_to_unchanged_recommendations(tmp_path, rec, dtype, space):
    from fashionvisualexpl_recommend_amd import train_rec
    paths, n_new, _ = _cli_dataset(tmp_path, "vbpr" if rec == "bprmf" else rec)
    I, K = 60, 5
    common = ["--rec", rec, "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--embed_color", "4", "--embed_edges", "6", "--reg", "0.01", "--top_k", "10", "--lr", "0.01",
              "--dtype", dtype]
    sim = ["--similar_items", str(K)] + (["--similar_space", space] if space else [])
    runs = [[], sim] + ([["--new_items"] + paths, sim + ["--new_items"] + paths] if rec != "bprmf" else [])
    res = [str(tmp_path / ("res%d" % q)) for q in range(len(runs))]
    for r, extra in zip(res, runs):
        train_rec.train(common + ["--results_root", r] + extra)
    rdir = [os.path.join(r, "rec_results", "toy", rec) for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] if "sim-" in f]
    assert [f for f in files[1] if "sim-" not in f] == files[0]
    base = [f for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(base) == 2
    for f in base:
        assert open(os.path.join(rdir[0], f), "rb").read() == open(os.path.join(rdir[1], f), "rb").read(), f
        s = f.replace("recs-", "sim-", 1)
        assert s in files[1]
        _well_formed(_rows(os.path.join(rdir[1], s)), I, K, I, no_self=True)
        if rec == "bprmf":
            continue
        assert [g for g in files[3] if "sim-" not in g] == files[2] and not [g for g in files[2] if "sim-" in g]
        new, ns = f.replace("recs-", "new-recs-", 1), f.replace("recs-", "new-sim-", 1)
        for g in (f, new):                                         # the bytes of the run without the flag
            assert open(os.path.join(rdir[2], g), "rb").read() == open(os.path.join(rdir[3], g), "rb").read(), g
        assert open(os.path.join(rdir[1], s), "rb").read() == open(os.path.join(rdir[3], s), "rb").read()
        assert ns in files[3] and ns not in files[1]
        _well_formed(_rows(os.path.join(rdir[3], ns)), n_new, K, I, no_self=False)
    assert any(f.startswith("best-sim-") for f in files[1])
    assert rec == "bprmf" or any(f.startswith("best-new-sim-") for f in files[3])
