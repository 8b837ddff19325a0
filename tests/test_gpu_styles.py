"""Style clusters on the MI355X: bprx_style_assign / bprx_style_update against the float64 restatement (tests/styles_ref.py), the
model methods on top of them and the files of train_rec --styles.

Assignment: tol(w) = (w + 4) 2^-23 (styles_ref.tol: the float32 fma chain over w products of vectors of norm <= 1, plus the norm
factor, doubled).  cos and second lie within tol of the reference; the style equals the reference's on every row whose reference
gap is >= 2 tol, a row below that is excused from the equality only (its choice still scores >= best - 2 tol), and at most 1 %
of a case's rows may be excused (tests/test_styles_cpu.py checks that the inputs used here excuse none).  The update is one
float32 rounding of a float64 result: 2^-23 per centroid component, size x 2^-23 for a mass.  Ties, special rows, the
invariances and the state are checked bit for bit."""
import gc
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import styles_ref as sr
from fashionvisualexpl_recommend_amd import _ffi, ranking, synth
from test_gpu_feat_explain import _bits, _unique_batches, _vbpr
from test_gpu_new_items import _cli_dataset

pytestmark = pytest.mark.gpu

U = 4


def _latent(z):
    """A BPRMF handle whose latent item space is z [I, w]."""
    from fashionvisualexpl_recommend_amd.engine import Engine
    I, w = z.shape
    e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=w, optimizer="sgd", lr=0.05, reg=0.0, max_batch=64)
    return e.bind(np.zeros((U, w), np.float32), z, np.zeros(I, np.float32))


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _assign(e, space, cent, q0=0, q1=None, rn=None, **kw):
    rn = e.sim_rnorm(space) if rn is None else rn
    out = e.style_assign(space, _dev(cent), q0, e.I if q1 is None else q1, rn, **kw)
    return tuple(None if x is None else x.cpu().numpy() for x in out)


def _check_assign(what, z, cent, got, rows=None):
    """The three outputs against the float64 reference under the rules of the module docstring."""
    w = z.shape[1]
    tol = sr.tol(w)
    rn = sr.rnorm(z)
    style, best, second, gap = (x if rows is None else x[rows] for x in sr.assign(z, rn, cent))
    g_style, g_cos, g_second = got
    c = sr.cosines(z, rn, cent)
    c = c if rows is None else c[rows]
    dev_c = np.abs(g_cos - best).max()
    finite = np.isfinite(second)
    assert np.array_equal(np.isneginf(g_second), np.isneginf(second))
    dev_s = np.abs(g_second[finite] - second[finite]).max() if finite.any() else 0.0
    exc = sr.excused(gap, w)
    print("%s: |cos - ref| %.3g, |second - ref| %.3g, tol %.3g, excused %d of %d" % (what, dev_c, dev_s, tol, exc.sum(), exc.size))
    assert dev_c <= tol and dev_s <= tol
    assert np.array_equal(g_style[~exc], style[~exc])
    assert exc.mean() <= 0.01
    live = g_style >= 0
    assert (c[np.flatnonzero(live), g_style[live]] >= best[live] - 2 * tol).all()


# ---- 1. assignment against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,w,S", sr.ASSIGN_CASES)
def test_assign_against_float64(I, w, S):
    z, cent = sr.assign_case(I, w, S)
    e = _latent(z)
    got = _assign(e, "latent", cent)
    assert got[0].dtype == np.int32 and all(x.shape == (I,) for x in got)
    _check_assign("I=%d w=%d S=%d" % (I, w, S), z, cent, got)
    e.sync_check()
    e.close()


def _both_engine():
    """The VBPR handle of styles_ref.both_case (fp32 features, one non-zero power of two per feature row: exact projections)."""
    Gi, F, E, z, cent = sr.both_case()
    I, k, d, _ = sr.BOTH_CASE
    rs = np.random.RandomState(78)
    t = dict(Gu=synth.glorot_uniform(rs, U, k), Gi=Gi, Bi=np.zeros(I, np.float32), Tu=synth.glorot_uniform(rs, U, d), F=F, E=E,
             Bp=np.zeros(sr.BOTH_FEAT, np.float32))
    return _vbpr(t, "fp32"), F, z, cent


def test_assign_both_spaces_and_caller_rows():
    """w = 40 = 24 + 16 on a VBPR handle, S = 257; then the visual space: the catalogue against the Pq form run on the catalogue's
    own projected rows."""
    e, F, z, cent = _both_engine()
    I, k, d, S = sr.BOTH_CASE
    e.sim_rnorm("both")
    assert np.array_equal(_bits(e.item_proj().cpu().numpy()[:, :d]), _bits(z[:, k:])), "the projections are not the planned ones"
    _check_assign("both", z, cent, _assign(e, "both", cent))
    zv, cv = z[:, k:], sr.unit_rows(np.random.RandomState(79), 130, d)
    cat = _assign(e, "visual", cv)
    _check_assign("visual", zv, cv, cat)
    P = e.project_rows(F)
    rq = e.sim_rnorm("visual", P)
    rows = e.style_assign("visual", _dev(cv), 0, I, rq, P, rq)
    rows = tuple(x.cpu().numpy() for x in rows)
    _check_assign("visual, Pq", zv, cv, rows)
    far = ~sr.excused(sr.assign(zv, sr.rnorm(zv), cv)[3], d)
    assert np.array_equal(rows[0][far], cat[0][far]) and np.abs(rows[1] - cat[1]).max() <= sr.tol(d)
    part = e.style_assign("visual", _dev(cv), 100, 300, rq, P, rq)
    assert all(np.array_equal(_bits(a.cpu().numpy()), _bits(b[100:300])) for a, b in zip(part, rows))
    e.sync_check()
    e.close()


# ---- 2. ties and special rows (exact) ----------------------------------------------------------------------------------------
def test_ties_and_special_rows():
    I, w, S = 300, 12, 140
    rs = np.random.RandomState(5)
    z = rs.standard_normal((I, w)).astype(np.float32)
    z[19] = z[7]                                               # bit-equal rows
    z[5] = 0                                                   # a zero row
    cent = sr.unit_rows(rs, S, w)
    cent[131] = cent[3]                                        # bit-equal centroids, in two tiles
    cent[64] = cent[40]                                        # ... and in the two column waves of one tile
    cent[41] = cent[40]                                        # ... and in two lanes of one wave
    cent[100] = 0                                              # a zero centroid
    e = _latent(z)
    style, cos, second = _assign(e, "latent", cent)
    assert not np.isin(style, [131, 64, 41]).any(), "a tie did not go to the smaller index"
    ref = sr.assign(z, sr.rnorm(z), cent)
    twin = np.isin(ref[0], [3, 40])
    assert twin.any() and np.array_equal(style[twin], ref[0][twin])
    assert np.array_equal(_bits(cos[twin]), _bits(second[twin])), "the twin's cosine is the second"
    assert all(np.array_equal(_bits(x[19:20]), _bits(x[7:8])) for x in (style, cos, second))
    assert (style[5], _bits(cos)[5], _bits(second)[5]) == (-1, 0, 0)
    # the zero centroid scores exactly 0.0: alone ...
    only = _assign(e, "latent", np.zeros((1, w), np.float32))
    live = np.arange(I) != 5
    assert (only[0][live] == 0).all() and (_bits(only[1]) == 0).all() and np.isneginf(only[2][live]).all() and only[2][5] == 0.0
    # ... and next to a centroid every row dislikes or likes
    pair = np.stack([np.zeros(w, np.float32), cent[0]])
    st2, cos2, sec2 = _assign(e, "latent", pair)
    neg = live & (sr.cosines(z, sr.rnorm(z), pair)[:, 1] < -1e-3)
    assert neg.any() and (st2[neg] == 0).all() and (cos2[neg] == 0.0).all()
    pos = live & (sr.cosines(z, sr.rnorm(z), pair)[:, 1] > 1e-3)
    assert (st2[pos] == 1).all() and (sec2[pos] == 0.0).all()
    # S = 1: second is -inf; second = NULL leaves style and cos alone
    one = _assign(e, "latent", cent[:1])
    assert np.isneginf(one[2][live]).all()
    s3, c3, none = _assign(e, "latent", cent, want_second=False)
    assert none is None and np.array_equal(s3, style) and np.array_equal(_bits(c3), _bits(cos))
    e.sync_check()
    e.close()


# ---- 3. invariance (bit-exact) -----------------------------------------------------------------------------------------------
def test_ranges_and_centroid_order_leave_a_rows_bits_alone():
    I, w, S = 389, 17, 300
    z, cent = sr.assign_case(I, w, S)
    e = _latent(z)
    rn = e.sim_rnorm("latent")
    whole = _assign(e, "latent", cent, rn=rn)
    for q0, q1 in [(0, 1), (0, 127), (0, 128), (127, 129), (1, 130), (128, 389), (388, 389), (200, 200)]:
        part = _assign(e, "latent", cent, q0, q1, rn=rn)
        assert all(p.shape == (q1 - q0,) and np.array_equal(_bits(p), _bits(x[q0:q1])) for p, x in zip(part, whole)), (q0, q1)
    guard = torch.full((64,), 7, dtype=torch.int32, device="cuda")   # q0 == q1 writes nothing
    lib, p = _ffi.lib(), lambda t: t.data_ptr()
    ct = _dev(cent)
    assert lib.bprx_style_assign(e.h, 0, None, I, 5, 5, p(rn), p(ct), S, p(guard), p(guard), p(guard), None) == 0
    assert (guard == 7).all()
    perm = np.random.RandomState(6).permutation(S)             # centroid s moves to row perm[s]
    moved = np.empty_like(cent)
    moved[perm] = cent
    st, cos, sec = _assign(e, "latent", moved, rn=rn)
    assert np.array_equal(st, perm[whole[0]]) and np.array_equal(_bits(cos), _bits(whole[1])) and np.array_equal(_bits(sec), _bits(whole[2]))
    e.sync_check()
    e.close()


# ---- 4. update against float64 -------------------------------------------------------------------------------------------------
def _update(e, rn, members, prev):
    S = len(members)
    ptr = np.zeros(S + 1, np.int64)
    np.cumsum([len(m) for m in members], out=ptr[1:])
    items = np.concatenate([np.asarray(m, np.int64) for m in members] + [np.zeros(1, np.int64)]).astype(np.int32)
    cent, mass = e.style_update("latent", rn, (_dev(ptr, torch.int64), _dev(items, torch.int32), S), _dev(prev))
    return cent.cpu().numpy(), mass.cpu().numpy()


def test_update_against_float64():
    I, w = 1300, 70                                            # two 64-column strips
    rs = np.random.RandomState(8)
    centre = rs.standard_normal(w)
    z = ((centre + 0.6 * rs.standard_normal((I, w))) * rs.uniform(0.5, 2.0, size=(I, 1))).astype(np.float32)
    z[1201] = -z[1200]                                           # a row and its exact negation
    e = _latent(z)
    rn = e.sim_rnorm("latent")
    rn_h = rn.cpu().numpy()
    sizes = [0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 1025]     # (16: a piece of the fixed order, 64: a round of four pieces)
    members = [np.sort(rs.choice(1100, n, replace=False)) for n in sizes] + [np.arange(I), np.array([1200, 1201])]
    S = len(members)
    prev = sr.unit_rows(rs, S, w)
    cent, mass = _update(e, rn, members, prev)
    ref_c, ref_m = sr.update(z, rn_h, members, prev)
    for s, m in enumerate(members):
        assert ref_m[s] == 0 or ref_m[s] >= 0.1 * len(m)
    dev_c = np.abs(cent - ref_c).max()
    dev_m = np.abs(mass - ref_m) / np.maximum(1, [len(m) for m in members])
    print("update: |cent - ref| %.3g (2^-23 = %.3g), |mass - ref| / size %.3g" % (dev_c, 2.0 ** -23, dev_m.max()))
    assert dev_c <= 2.0 ** -23 and (dev_m <= 2.0 ** -23).all()
    assert (mass >= 0).all() and (mass <= np.array([len(m) for m in members]) * (1 + 2.0 ** -22)).all()
    for s in (0, S - 1):                                       # the empty cluster and the cancelling pair keep their row
        assert np.array_equal(_bits(cent[s]), _bits(prev[s])) and mass[s] == 0.0
    again = _update(e, rn, members, prev)
    assert np.array_equal(_bits(again[0]), _bits(cent)) and np.array_equal(_bits(again[1]), _bits(mass))
    order = rs.permutation(S)                                  # the same clusters under other indices, among other clusters
    other = [members[s] for s in order] + [np.arange(3, 40)]
    c2, m2 = _update(e, rn, other, np.concatenate([prev[order], prev[:1]]))
    assert np.array_equal(_bits(c2[:S]), _bits(cent[order])) and np.array_equal(_bits(m2[:S]), _bits(mass[order]))
    e.sync_check()
    # a member outside the catalogue is skipped and reported; the handle works afterwards
    bad = [np.array([-1, 3, 8, I]), members[5]]
    c3, m3 = _update(e, rn, bad, prev[:2])
    with pytest.raises(_ffi.BprxError) as err:
        e.sync_check()
    assert err.value.code == _ffi.E_RANGE
    e.sync_check()
    good = _update(e, rn, [np.array([3, 8]), members[5]], prev[:2])
    assert np.array_equal(_bits(c3), _bits(good[0])) and np.array_equal(_bits(m3), _bits(good[1]))
    assert np.array_equal(_bits(good[0][1]), _bits(cent[5]))
    e.sync_check()
    e.close()


# ---- 5. the loop ---------------------------------------------------------------------------------------------------------------
def _params(rec, opt="sgd", **kw):
    return Namespace(dataset="toy", validation=True, batch_size=64, epochs=1, batch_eval=128, embed_k=16, embed_d=12, lr=0.05,
                     reg=1e-3, top_k=10, verbose=-1, restore_epochs=1, rec=rec, best_metric="ndcg", optimizer=opt, init_seed=5,
                     dtype="bf16", **kw)


def test_the_loop_recovers_planted_styles():
    from fashionvisualexpl_recommend_amd.models import BPRMF
    z, label = sr.planted([1, 40, 64, 65, 130, 300], 16, 0.05, seed=3)
    I = z.shape[0]
    tr, va, te = synth.make_interactions(20, I, per_user=8, seed=9)
    data = Namespace(training_list=tr, validation_list=va, test_list=te, num_users=20, num_items=I, params=_params("bprmf"))
    m = BPRMF(data, _params("bprmf", styles=6), init={"Gi": z})
    rn = m.engine.sim_rnorm("latent").cpu().numpy()
    seeds = m.style_seeds(6)
    assert seeds.dtype == np.int64 and np.array_equal(seeds, sr.seeds(z, rn, 6))
    style, cos, cent, obj = m.item_styles()
    r_style, r_cos, r_cent, r_obj = sr.loop(z, rn, 6)
    print("loop: %d iterations, objective %s" % (len(obj), obj))
    assert style.dtype == np.int64 and cos.dtype == np.float32 and cent.shape == (6, 16) and obj.dtype == np.float64
    assert np.array_equal(style, r_style) and sr.same_partition(style, label)
    assert len(obj) < 20 and len(obj) == len(r_obj) and (np.diff(obj) >= -sr.tol(16)).all()
    assert np.abs(cos - r_cos).max() <= sr.tol(16) and np.abs(obj - r_obj).max() <= sr.tol(16)
    assert np.abs(cent - r_cent).max() <= 2.0 ** -22
    poor = np.arange(6)                                        # seeds that start far from the planted centres: several iterations
    p_style, p_cos, p_cent, p_obj = m.item_styles(seeds=poor)
    q_style, q_cos, q_cent, q_obj = sr.loop(z, rn, 6, seed_ids=poor)
    print("loop from items 0..5: %d iterations, objective %s" % (len(p_obj), p_obj))
    assert np.array_equal(p_style, q_style) and len(p_obj) == len(q_obj) and 1 < len(p_obj) < 20
    assert (np.diff(p_obj) >= -sr.tol(16)).all() and np.abs(p_obj - q_obj).max() <= sr.tol(16)
    sizes, ids, vals, cnt = m.style_members(style, cos, top=3)
    assert np.array_equal(sizes, np.bincount(style, minlength=6)) and np.array_equal(cnt, np.minimum(sizes, 3))
    for s in range(6):
        mine = np.flatnonzero(style == s)
        want = mine[np.lexsort((mine, -cos[mine]))][:3]
        assert np.array_equal(ids[s, :cnt[s]], want) and np.array_equal(_bits(vals[s, :cnt[s]]), _bits(cos[want]))
    with pytest.raises(ValueError):
        m.style_seeds(I + 1)
    m.engine.close()


# ---- 6. state ------------------------------------------------------------------------------------------------------------------
def test_calls_between_steps_leave_the_run_bit_identical(monkeypatch):
    """A VBPR handle with lazy Adam and the deferred dense update (the engines and batches of tests/test_gpu_dense_defer.py):
    item_styles and the two entry points run between two steps, while an update is pending and rows lag; the run ends bit-equal
    to one without the calls."""
    import test_gpu_dense_defer as dd
    from fashionvisualexpl_recommend_amd.models import VBPR
    lib = _ffi.lib()
    I, k = dd.I, dd.K
    batches = [dd._batch(300 + s) for s in range(6)]
    end = []
    for with_call in (False, True):
        e = dd._engine(monkeypatch, True, 256, 20, "bf16", "lazy")
        assert e.adam_is_lazy()
        m = object.__new__(VBPR)                               # the model's style methods on this engine (no data, no evaluator)
        m.engine, m.num_items, m.similar_space, m.styles_S, m.style_iters = e, I, "visual", 0, 20
        for s, b in enumerate(batches):
            if s == 3 and with_call:
                assert e.dense_pending()
                for space in ("both", "visual"):
                    style, cos, cent, obj = m.item_styles(S=5, iters=4, space=space)
                    assert style.min() >= 0 and style.max() < 5 and len(obj) >= 1
                assert not e.dense_pending()
                rn = e.sim_rnorm("visual")
                ct = _dev(cent)
                live = lib.bprx_live_device_allocs()
                st, _, _ = e.style_assign("visual", ct, 0, I, rn)
                assert lib.bprx_live_device_allocs() == live
                e.style_update("visual", rn, ranking.class_csr(st.cpu().numpy(), I, e.device, classes=5), ct)
                assert lib.bprx_live_device_allocs() == live
            if s == 4 and with_call:                           # ... and once more with the update of step 3 pending
                assert e.dense_pending()
                live = lib.bprx_live_device_allocs()
                rn = e.sim_rnorm("both")
                cb = _dev(sr.unit_rows(np.random.RandomState(1), 7, k + 20))
                st, _, _ = e.style_assign("both", cb, 0, I, rn)
                e.style_update("both", rn, ranking.class_csr(st.cpu().numpy(), I, e.device, classes=7), cb)
                assert not e.dense_pending()
                del rn, cb, st
            e.step(*b, want_loss=False)
        e.sync_check()
        end.append({n: v.cpu().numpy() for n, v in e.t.items() if n != "F" and v is not None})
        e.close()
    for n in end[0]:
        a, b = (np.ascontiguousarray(x[n]) for x in end)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), n


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable():
    from fashionvisualexpl_recommend_amd.engine import Engine
    from test_gpu_feat_explain import _tables
    lib = _ffi.lib()
    gc.collect()
    p = lambda t: None if t is None else t.data_ptr()
    I, k, d = 80, 16, 12
    t = _tables(50, I, k, d, 256, 200, "bf16", seed=20)
    v = _vbpr(t, "bf16")
    m = Engine(model="bprmf", num_users=50, num_items=I, embed_k=k, optimizer="sgd", lr=0.05, reg=0.0, max_batch=64)
    m.bind(t["Gu"], t["Gi"], t["Bi"])
    f8 = _vbpr(t, "fp8")
    unbound = Engine(model="bprmf", num_users=50, num_items=I, embed_k=k, optimizer="sgd", lr=0.05, reg=0.0, max_batch=64)
    S = 3
    st = torch.empty(I, dtype=torch.int32, device="cuda")
    cs, sc, ms = (torch.empty(I, dtype=torch.float32, device="cuda") for _ in range(3))
    ptr, items, _ = ranking.class_csr(np.arange(I) % S, I, "cuda", classes=S)
    P = v.project_rows(t["F"][:10])

    def assign(e, space=0, Pq=None, nq=I, q0=0, q1=I, rn=cs, cent="zeros", S=S, style=st, cos=cs, second=sc, w=k):
        cent = torch.zeros((max(S, 1), w), dtype=torch.float32, device="cuda") if cent == "zeros" else cent
        return lib.bprx_style_assign(e.h if e else None, space, p(Pq), nq, q0, q1, p(rn), p(cent), S, p(style), p(cos), p(second), None)

    def update(e, space=0, rn=cs, mp=ptr, mi=items, S=S, prev="zeros", out="zeros", mass=ms, w=k):
        z = [torch.zeros((max(S, 1), w), dtype=torch.float32, device="cuda") for _ in range(2)]
        prev, out = (z[q] if x == "zeros" else x for q, x in enumerate((prev, out)))
        return lib.bprx_style_update(e.h if e else None, space, p(rn), p(mp), p(mi), S, p(prev), p(out), p(mass), None)

    def usable(e, space=0, w=k):
        assert assign(e, space, w=w) == 0 and update(e, space, w=w) == 0
        e.sync_check()

    usable(v), usable(m), usable(v, 1, d), usable(v, 2, k + d), usable(f8)
    assert assign(None) == _ffi.E_INVALID and update(None) == _ffi.E_INVALID
    cases = [(v, lambda e: assign(e, rn=None)), (v, lambda e: assign(e, cent=None)), (v, lambda e: assign(e, style=None)),
             (v, lambda e: assign(e, cos=None)), (v, lambda e: assign(e, S=0)), (v, lambda e: assign(e, S=1025)),
             (v, lambda e: assign(e, space=3)), (v, lambda e: assign(e, space=-1)), (m, lambda e: assign(e, space=1)),
             (m, lambda e: assign(e, space=2)), (f8, lambda e: assign(e, space=1)), (f8, lambda e: assign(e, space=2)),
             (v, lambda e: assign(e, q0=-1)), (v, lambda e: assign(e, q0=5, q1=4)), (v, lambda e: assign(e, q1=I + 1)),
             (v, lambda e: assign(e, nq=I - 1, q1=I - 1)), (v, lambda e: assign(e, space=0, Pq=P, nq=10, q1=10)),
             (v, lambda e: assign(e, space=2, Pq=P, nq=10, q1=10)), (m, lambda e: assign(e, space=1, Pq=P, nq=10, q1=10)),
             (v, lambda e: update(e, rn=None)), (v, lambda e: update(e, mp=None)), (v, lambda e: update(e, mi=None)),
             (v, lambda e: update(e, prev=None)), (v, lambda e: update(e, out=None)), (v, lambda e: update(e, mass=None)),
             (v, lambda e: update(e, S=0)), (v, lambda e: update(e, S=1025)), (v, lambda e: update(e, space=3)),
             (m, lambda e: update(e, space=1)), (m, lambda e: update(e, space=2)), (f8, lambda e: update(e, space=1))]
    for q, (e, call) in enumerate(cases):
        assert call(e) == _ffi.E_INVALID, q
        assert lib.bprx_last_error(e.h)
        usable(e)
    assert assign(unbound) == _ffi.E_STATE and update(unbound) == _ffi.E_STATE
    unbound.bind(t["Gu"], t["Gi"], t["Bi"])
    usable(unbound)
    assert assign(v, space=1, Pq=P, nq=10, q1=10, w=d) == 0 and assign(v, second=None) == 0
    with pytest.raises(_ffi.BprxError) as err:
        m.style_assign("visual", torch.zeros((2, k), dtype=torch.float32, device="cuda"), 0, I, cs)
    assert err.value.code == _ffi.E_INVALID
    usable(m)
    # ACF and AttentiveFashion handles have no item space of this kind
    import attentive_ref
    import test_gpu_acf as ga
    import test_gpu_attentive as gaf
    from acf_ref import random_tables
    rs = np.random.RandomState(64)
    acf = ga._engine(random_tables(rs, 12, I, k, 128, 64, 64, scale=10.0), ga._features(rs, I, 9, 128, "fp32"),
                     ga._lists(rs, 12, I, rs.randint(0, 15, 12)))
    af = gaf._engine(attentive_ref.random_tables(rs, 12, I, k, 8, 6, 64), attentive_ref.random_inputs(rs, I, 8, 6))
    for e in (acf, af):
        assert assign(e) == _ffi.E_INVALID and update(e) == _ffi.E_INVALID
        e.sync_check()
    for e in (v, m, f8, unbound, acf, af):
        e.sync_check()
        e.close()


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------
def _rows(path):
    return [l.rstrip("\n").split("\t") for l in open(path)]


@pytest.mark.parametrize("rec", ["vbpr", "bprmf"])
def test_cli_writes_the_style_files_next_to_unchanged_recommendations(tmp_path, rec):
    from fashionvisualexpl_recommend_amd import train_rec
    paths, n_new, _ = _cli_dataset(tmp_path, "vbpr")                 # 30 users, 60 items
    Un, I, S, top = 30, 60, 5, 3
    # --batch_size 1: a step adds at most one term to a gradient row, so runs of the same seed agree bit for bit
    common = ["--rec", rec, "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--reg", "0.01", "--top_k", "10", "--lr", "0.01", "--optimizer", "sgd", "--dtype", "bf16"]
    flags = ["--styles", str(S), "--style_top", str(top), "--item_classes", "styles", "--shelves", "3", "--class_cap", "2"]
    flags += ["--new_items"] + paths if rec == "vbpr" else ["--similar_space", "latent"]
    res = [str(tmp_path / ("res%d" % q)) for q in range(2)]
    rdir = [os.path.join(r, "rec_results", "toy", rec) for r in res]
    train_rec.train(common + flags + ["--results_root", res[0]])
    m = train_rec._last_model
    train = [list(l) for l in m.data.training_list[:Un]]
    m.engine.close()
    train_rec.train(common + ["--results_root", res[1]])
    train_rec._last_model.engine.close()
    with_flags, without = sorted(os.listdir(rdir[0])), sorted(os.listdir(rdir[1]))
    assert not [f for f in without if "style" in f or "shelf" in f or "cap-" in f]
    for f in without:
        if f.startswith(("recs-", "best-recs-")):
            assert open(os.path.join(rdir[0], f), "rb").read() == open(os.path.join(rdir[1], f), "rb").read(), f
    kinds = ["styles", "style-items", "user-styles", "shelf-recs", "cap-recs"] + (["new-styles"] if rec == "vbpr" else [])
    for head in ("recs-", "best-recs-"):
        base = [f for f in without if f.startswith(head)]
        assert len(base) == 1
        best, tail = ("best-", base[0][len("best-recs"):]) if head == "best-recs-" else ("", base[0][len("recs"):])
        for kind in kinds:
            assert best + kind + tail in with_flags, kind
        rd = lambda kind: _rows(os.path.join(rdir[0], best + kind + tail))
        st = rd("styles")
        assert [int(r[0]) for r in st] == list(range(I)) and all(-1 <= int(r[1]) < S for r in st)
        style = np.array([int(r[1]) for r in st])
        cos = np.array([np.float32(r[2]) for r in st])
        sizes = np.bincount(style[style >= 0], minlength=S)
        by_style = {}
        for s, size, rank, i, c in rd("style-items"):
            assert style[int(i)] == int(s) and int(size) == sizes[int(s)] and np.float32(c) == cos[int(i)]
            by_style.setdefault(int(s), []).append((int(rank), int(i)))
        for s in range(S):
            mine = np.flatnonzero(style == s)
            want = mine[np.lexsort((mine, -cos[mine]))][:top]
            assert [i for _, i in by_style.get(s, [])] == want.tolist() and [r for r, _ in by_style.get(s, [])] == list(range(len(want)))
        owned = {}
        last = {}
        for u, s, n, share in rd("user-styles"):
            u, s, n = int(u), int(s), int(n)
            assert n == sum(style[i] == s for i in train[u]) and np.float32(share) == np.float32(n) / np.float32(len(train[u]))
            assert u not in last or (last[u][0] > n or (last[u][0] == n and last[u][1] < s))
            last[u] = (n, s)
            owned[u] = owned.get(u, 0) + n
        assert all(owned.get(u, 0) == sum(style[i] >= 0 for i in train[u]) for u in range(Un))
        assert (style >= 0).all() and all(owned[u] == len(train[u]) for u in range(Un))
        shelf, cap = rd("shelf-recs"), rd("cap-recs")
        assert shelf and cap
        assert all(int(r[1]) == style[int(r[2])] for r in shelf) and all(int(r[3]) == style[int(r[1])] for r in cap)
        if rec == "vbpr":
            new = rd("new-styles")
            assert [int(r[0]) for r in new] == list(range(n_new)) and all(-1 <= int(r[1]) < S for r in new)
