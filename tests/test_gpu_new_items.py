"""Scoring, ranking and explaining items the model was not trained on, on the MI355X, against the float64 restatement
(tests/new_items_ref.py): bprx_project_rows, bprx_score_new_block, bprx_topk_rows, bprx_feat_explain_new, the model methods on top
of them and the files of train_rec --new_items.

Allowance per compared output (the rule of tests/test_gpu_feat_explain.py): 32 x the max-abs deviation of the FLOAT32 restatement
from the float64 one over the case, never below one float32 ulp of the output's largest magnitude.  Every check prints its triple
(float32 deviation / allowance / GPU deviation).  What is exact is checked exactly: the padding columns, the words behind an
output, a row's bits wherever it stands, two calls, the lists against the GPU's own rows.

GradFashion: with fp32 features the float64 reference is tests/gradfashion_ref.py's visual term itself.  With bf16 features the
library multiplies with the bf16 rounding of the E_eff it composed in fp32; rounding a float64 E_eff instead moves single elements
by a whole bf16 step (2^-9 relative, far above any float32 allowance) wherever the two compositions fall on different sides of a
rounding boundary.  So there the restatement takes the handle's own E_eff / Bp_eff (as test_gpu_feat_explain's factored case
does), E_eff / Bp_eff are held against gradfashion_ref's effective(), and gradfashion_ref's visual term against the project's
bf16 bound (2^-8 x the sum of the absolute terms)."""
import gc
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import new_items_ref as N
from fashionvisualexpl_recommend_amd import _ffi, synth
from gradfashion_ref import GradFashionRef
from oracle import oracle as orc
from test_gpu_feat_explain import _bits, _snapshot, _tables, _unique_batches, _vbpr
from test_gpu_gradfashion import Dc, De, PAD, _engine as _gf_engine, _setup as _gf_setup

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 12345.678


def _allow(r64, r32):
    """(float32 deviation, allowance) of one output over a case."""
    dev = float(np.abs(r64 - r32.astype(np.float64)).max())
    return dev, max(32.0 * dev, float(np.spacing(np.float32(np.abs(r64).max()))))


def _report(tag, r64, r32, got):
    dev, allow = _allow(r64, r32)
    gdev = float(np.abs(got.astype(np.float64) - r64).max())
    print("%s: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (tag, dev, allow, gdev))
    return gdev, allow


def _new_rows(n, D, ncols, dtype, seed):
    """n feature rows of new items: `ncols` real columns (some above the training max-abs of 1), zero padding up to D."""
    F = np.zeros((n, D), np.float32)
    f = synth.make_features(n, ncols, seed=seed)
    F[:, :ncols] = f / np.abs(f).max() * 1.5
    return orc.bf16_round(F) if dtype == "bf16" else F


def _dev(e, F):
    return e._new_table(F)


def _project_guarded(e, Fd, n):
    """bprx_project_rows on the first n rows of the device table Fd into a buffer with a patterned tail, which must survive."""
    PS = e.proj_stride()
    buf = torch.full((n * PS + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    _ffi.check(e.h, e.lib.bprx_project_rows(e.h, Fd.data_ptr(), n, buf.data_ptr(), None))
    torch.cuda.synchronize()
    assert (buf[n * PS:] == PATTERN).all(), "project_rows wrote behind its %d x %d output" % (n, PS)
    return buf[:n * PS].view(n, PS).cpu().numpy()


# ---- projection --------------------------------------------------------------------------------------------------------------
SHAPES = [("bf16", D, d) for D in (128, 384) for d in (12, 15, 16, 20, 64)] + \
         [("fp32", D, d) for D in (128, 384, 40) for d in (12, 15, 16, 20, 64)]


@pytest.mark.parametrize("dtype,D,d", SHAPES)
def test_projection_edges(dtype, D, d):
    """One chunk and an odd chunk count; padding columns, d + 1 exactly one tile, Bp opening a second tile, the CLI default, five
    column tiles; less than a tile, a tile edge, more than a workgroup's rows.  fp32, D = 40: the form without the matrix unit."""
    t = _tables(130, 40, 8, d, D, D, dtype, seed=30)
    e = _vbpr(t, dtype)
    PS = 16 * ((d + 1 + 15) // 16)
    assert e.proj_stride() == PS
    F = _new_rows(300, D, D, dtype, seed=31)
    Fd = _dev(e, F)
    r64, r32 = (N.projection(F, t["E"], t["Bp"], dtype, dt) for dt in (torch.float64, torch.float32))
    dev, allow = _allow(r64, r32)
    for n in (1, 15, 16, 17, 33, 300):
        P = _project_guarded(e, Fd, n)
        gdev = float(np.abs(P[:, :d + 1] - r64[:n]).max())
        print("proj %s D=%d d=%d n=%d: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (dtype, D, d, n, dev, allow, gdev))
        assert gdev <= allow, (n, gdev, allow)
        assert (P[:, d + 1:] == 0).all(), "n=%d: padding columns" % n
    assert np.array_equal(_bits(e.project_rows(F).cpu().numpy()), _bits(_project_guarded(e, Fd, 300)))
    e.sync_check()
    e.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_a_rows_bits_do_not_depend_on_its_position_or_on_n(dtype):
    D, d = 384, 20
    t = _tables(130, 40, 8, d, D, D, dtype, seed=32)
    e = _vbpr(t, dtype)
    F = _new_rows(300, D, D, dtype, seed=33)
    spots = [0, 15, 16, 17, 299]
    F[spots] = F[123]
    P = e.project_rows(F).cpu().numpy()
    one = e.project_rows(F[123:124]).cpu().numpy()
    for r in spots + [123]:
        assert np.array_equal(_bits(P[r]), _bits(one[0])), r
    assert np.array_equal(_bits(P), _bits(e.project_rows(F).cpu().numpy())), "two calls differ"
    assert len({P[r].tobytes() for r in range(300)}) == 300 - len(spots)        # (the other rows are all different)
    e.close()


# ---- scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 512), ("fp32", 400)])
def test_new_and_catalogue_items_are_on_one_scale(dtype, D):
    """Gi = 0, Bi = 0 and the bound table's own rows as the new table: score_block and score_new_block restate the same float64
    values (no bit equality: the catalogue's tiled kernels sum in another order)."""
    U, I, d = 130, 300, 20
    t = _tables(U, I, 8, d, D, 390, dtype, seed=34)
    t["Gi"][:], t["Bi"][:] = 0, 0
    e = _vbpr(t, dtype)
    new = e.score_new_block(0, U, e.project_rows(t["F"])).cpu().numpy()
    cat = e.score_block(0, U).cpu().numpy()
    r64, r32 = (N.scores(t["Tu"], t["F"], t["E"], t["Bp"], 0, U, dtype, dt) for dt in (torch.float64, torch.float32))
    g_new, allow = _report("one scale %s new" % dtype, r64, r32, new)
    g_cat, _ = _report("one scale %s catalogue" % dtype, r64, r32, cat)
    assert g_new <= allow and g_cat <= allow
    e.sync_check()
    e.close()


@pytest.mark.parametrize("d", [15, 20])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_score_block_edges(dtype, d):
    U, D = 130, 128
    t = _tables(U, 40, 8, d, D, D, dtype, seed=35)
    e = _vbpr(t, dtype)
    F = _new_rows(300, D, D, dtype, seed=36)
    r64, r32 = (N.scores(t["Tu"], F, t["E"], t["Bp"], 0, U, dtype, dt) for dt in (torch.float64, torch.float32))
    allow = _allow(r64, r32)[1]
    for n in (1, 127, 129, 300):
        P = e.project_rows(F[:n])
        for u0, u1 in ((0, 1), (0, 130), (127, 130)):
            nu = u1 - u0
            buf = torch.full((nu * n + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
            got = e.score_new_block(u0, u1, P, out=buf[:nu * n].view(nu, n)).cpu().numpy()
            assert (buf[nu * n:] == PATTERN).all()
            gdev = float(np.abs(got - r64[u0:u1, :n]).max())
            print("scores %s d=%d n=%d [%d,%d): allowance %.3e / GPU deviation %.3e" % (dtype, d, n, u0, u1, allow, gdev))
            assert gdev <= allow
    assert e.score_new_block(5, 5, P).shape == (0, 300)
    e.sync_check()
    e.close()


# ---- top-K -------------------------------------------------------------------------------------------------------------------
def _expected_lists(S, K):
    """(idx, val, flag) of bprx_topk's rules for the rows of S, on the CPU: (value descending, index ascending); a row is flagged
    when K exceeds the width, or equal values meet inside the list or at its boundary."""
    nrows, width = S.shape
    Kc = min(K, width)
    idx, val = np.full((nrows, K), -1, np.int32), np.zeros((nrows, K), np.float32)
    flag = np.zeros(nrows, np.int32)
    for r in range(nrows):
        order = np.lexsort((np.arange(width), -S[r].astype(np.float64)))
        v = S[r][order]
        idx[r, :Kc], val[r, :Kc] = order[:Kc], v[:Kc]
        flag[r] = int(K > width or (v[:Kc - 1] == v[1:Kc]).any() or (Kc < width and v[Kc - 1] == v[Kc]))
    return idx, val, flag


@pytest.mark.parametrize("K", [1, 5, 20])
@pytest.mark.parametrize("width", [1, 5, 300])
def test_topk_rows(width, K):
    """Lists of the GPU's own score rows.  width 300: the row the float64 restatement ranks 10th for user 0 is copied over the row
    it ranks last: bit-equal scores for every user, so user 0 is flagged whenever its list reaches rank 10, and so is exactly every
    user whose list or list boundary holds that pair -- and every row when K > width."""
    U, D, d = 130, 128, 20
    t = _tables(U, 40, 8, d, D, D, "bf16", seed=37)
    e = _vbpr(t, "bf16")
    F = _new_rows(width, D, D, "bf16", seed=38)
    if width == 300:
        order = np.argsort(-N.scores(t["Tu"], F, t["E"], t["Bp"], 0, 1, "bf16")[0], kind="stable")
        src, dst = int(order[9]), int(order[-1])
        F[dst] = F[src]
    S = e.score_new_block(0, U, e.project_rows(F))
    Sh = S.cpu().numpy()
    if width == 300:
        assert np.array_equal(_bits(Sh[:, src]), _bits(Sh[:, dst]))
    idx, val, flag = (x.cpu().numpy() for x in e.topk_rows(S, K))
    assert np.array_equal(_bits(S.cpu().numpy()), _bits(Sh)), "topk_rows masks nothing"
    widx, wval, wflag = _expected_lists(Sh, K)
    assert np.array_equal(flag, wflag), (np.nonzero(flag != wflag)[0][:10], flag.sum(), wflag.sum())
    ok = flag == 0
    assert np.array_equal(idx[ok], widx[ok]) and np.array_equal(_bits(val[ok]), _bits(wval[ok]))
    Kc = min(K, width)
    assert (idx[:, Kc:] == -1).all() and not _bits(val[:, Kc:]).any()
    if K > width:
        assert flag.all()
    elif width == 300:
        dup = np.array([src in widx[r] or dst in widx[r] or Sh[r, src] == wval[r, K - 1] for r in range(U)])
        assert np.array_equal(flag.astype(bool), dup) and flag[0] == (1 if K == 20 else 0)
    else:
        assert not flag.any()
    e.sync_check()
    e.close()


def _model(dtype="bf16", U=130, I=60, D=128, **kw):
    from fashionvisualexpl_recommend_amd.models import VBPR
    p = dict(dataset="vb", validation=True, batch_size=64, epochs=1, batch_eval=128, embed_k=8, embed_d=20, lr=2e-3, reg=1e-3,
             top_k=20, verbose=-1, restore_epochs=1, rec="vbpr", best_metric="ndcg", optimizer="sgd", init_seed=5, dtype=dtype)
    p.update(kw)
    p = Namespace(**p)
    tr, va, te = synth.make_interactions(U, I, per_user=8, seed=39)
    data = Namespace(num_users=U, num_items=I, training_list=tr, validation_list=va, test_list=te, params=p)
    raw = synth.make_features(I, D, seed=40) * 3.7
    return VBPR(data, p, features=raw), raw


def test_model_recommend_new_prepare_and_snapshot():
    m, raw = _model()
    assert float(m.feat_norm) == float(np.abs(raw).max())
    new_raw = np.concatenate([raw[[5, 9]], synth.make_features(48, 128, seed=41) * 5.0])
    order = np.argsort(-m.score_new_items(new_raw, 0, 1).cpu().numpy()[0], kind="stable")
    new_raw[order[-1]] = new_raw[order[9]]                         # one item twice, 10th for user 0: that list depends on the order of equals
    Fd = m.prepare_new_items(new_raw)
    assert Fd.dtype == torch.bfloat16 and Fd.is_cuda and tuple(Fd.shape) == (50, 128)
    assert torch.equal(Fd[:2].view(torch.int16), m.engine._t["F"][[5, 9]].view(torch.int16))    # equal raw rows: equal table rows
    assert float(Fd.float().max()) > 1.0
    with pytest.raises(ValueError):
        m.prepare_new_items(new_raw[:, :100])
    S = m.score_new_items(new_raw).cpu().numpy()
    assert S.shape == (130, 50) and np.array_equal(_bits(S[10:20]), _bits(m.score_new_items(Fd, 10, 20).cpu().numpy()))
    idx, val = m.recommend_new(new_raw, k=20)
    assert idx.shape == val.shape == (130, 20)
    _, _, wflag = _expected_lists(S, 20)
    assert wflag[0] == 1
    for r in range(130):
        if wflag[r]:                                               # numpy's order on the GPU's row, as store_recommendation does
            want = S[r].argsort()[-20:][::-1]
        else:
            want = np.lexsort((np.arange(50), -S[r].astype(np.float64)))[:20]
        assert np.array_equal(idx[r], want) and np.array_equal(_bits(val[r]), _bits(S[r][want])), r
    i2, v2, ex = m.recommend_new(new_raw, k=5, u0=3, u1=9, explain=4)
    assert i2.shape == (6, 5) and ex["col"].shape == (30, 4) and ex["score"].shape == (30,)
    direct = m.engine.feat_explain_new(Fd, np.repeat(np.arange(3, 9), 5), i2.reshape(-1), 4, 128)
    assert np.array_equal(ex["col"], direct["col"].cpu().numpy())
    sd = m.state_dict()
    assert sd["feat_norm"].dim() == 0 and float(sd["feat_norm"]) == float(m.feat_norm)
    kept = m.feat_norm
    m.feat_norm = None
    m.load_state_dict(sd)
    assert m.feat_norm == kept and m.feat_norm.dtype == kept.dtype
    m.load_state_dict({n: v for n, v in sd.items() if n != "feat_norm"})      # a snapshot from before the key
    assert m.feat_norm == kept
    m.engine.close()
    with pytest.raises(ValueError):
        _model("fp8", D=256)[0].prepare_new_items(np.ones((2, 256), np.float32))


# ---- explanations ------------------------------------------------------------------------------------------------------------
def _explain(e, Fd, u, r, top, ncols, maps):
    return {n: v.cpu().numpy() for n, v in e.feat_explain_new(Fd, u, r, top, ncols, maps=maps).items()}


def _same(a, b):
    return all(np.array_equal(_bits(a[n]), _bits(b[n])) for n in a if n in b) and (set(a) - {"map"}) == (set(b) - {"map"})


def _check_new(e, t, F, Fd, u, r, ncols, top, tag, pool=None):
    """The _check of tests/test_gpu_feat_explain.py for pairs (user, new row): there is no base, score is the visual sum."""
    u, r = np.asarray(u, np.int32), np.asarray(r, np.int32)
    n = len(u)
    got = _explain(e, Fd, u, r, top, ncols, True)
    assert _same(got, _explain(e, Fd, u, r, top, ncols, True)), tag + ": two calls differ"
    assert _same(got, _explain(e, Fd, u, r, top, ncols, False)), tag + ": the call without the map differs"
    e.sync_check()
    assert set(got) == {"score", "visual", "col", "contrib", "map"} and got["map"].shape == (n, ncols)
    assert np.array_equal(_bits(got["score"]), _bits(got["visual"]))
    r64 = N.explain(t["Tu"], F, t["E"], t["Bp"], u, r, ncols)
    pu, pr = (u, r) if pool is None else pool
    p64 = r64 if pool is None else N.explain(t["Tu"], F, t["E"], t["Bp"], pu, pr, ncols)
    p32 = N.explain(t["Tu"], F, t["E"], t["Bp"], pu, pr, ncols, torch.float32)
    kk = min(top, ncols)
    srt = lambda m: -np.sort(-m.astype(np.float64), axis=1, kind="stable")[:, :kk]
    allow = {"score": _allow(p64["score"], p32["score"]), "map": _allow(p64["map"], p32["map"]),
             "contrib": _allow(srt(p64["map"]), srt(p32["map"]))}
    rows = np.arange(n)[:, None]
    col, con = got["col"][:, :kk], got["contrib"][:, :kk]
    assert (col >= 0).all() and (col < ncols).all()
    dev = {"score": np.abs(got["score"] - r64["score"]), "map": np.abs(got["map"] - r64["map"]),
           "contrib": np.maximum(np.abs(con - r64["map"][rows, col]), np.abs(con - srt(r64["map"])))}
    for name in ("score", "map", "contrib"):
        print("%s %s: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (tag, name, allow[name][0], allow[name][1],
                                                                                          float(dev[name].max())))
    for name in ("score", "map", "contrib"):
        assert float(dev[name].max()) <= allow[name][1], (tag, name, float(dev[name].max()), allow[name])
    assert (con[:, :-1] >= con[:, 1:]).all()
    eq = con[:, :-1] == con[:, 1:]
    assert (col[:, :-1][eq] < col[:, 1:][eq]).all()
    assert (got["col"][:, kk:] == -1).all() and not _bits(got["contrib"][:, kk:]).any()
    assert np.array_equal(_bits(con), _bits(got["map"][rows, col]))
    assert np.array_equal(np.argsort(-got["map"], axis=1, kind="stable")[:, :kk], col), tag + ": not the stable sort of the map"
    return got


@pytest.mark.parametrize("dtype,D", [("bf16", 512), ("fp32", 400)])
def test_explanations_of_new_rows(dtype, D):
    U, n_new, ncols = 300, 600, 390
    t = _tables(U, 50, 16, 12, D, ncols, dtype, seed=42)
    e = _vbpr(t, dtype)
    F = _new_rows(n_new, D, ncols, dtype, seed=43)
    Fd = _dev(e, F)
    rs = np.random.RandomState(44)
    grouped = np.repeat(rs.randint(U, size=50), 20).astype(np.int32)
    rows = rs.randint(n_new, size=1000).astype(np.int32)
    perm = rs.permutation(1000)
    g = _check_new(e, t, F, Fd, grouped, rows, ncols, 32, "expl %s grouped" % dtype)
    s = _check_new(e, t, F, Fd, grouped[perm], rows[perm], ncols, 32, "expl %s shuffled" % dtype)
    for name in g:                                                  # a pair's outputs depend on the pair alone
        assert np.array_equal(_bits(s[name]), _bits(g[name][perm])), name
    one = _check_new(e, t, F, Fd, grouped[:1], rows[:1], ncols, 32, "expl %s n=1" % dtype, pool=(grouped, rows))
    for name in one:
        assert np.array_equal(_bits(one[name]), _bits(g[name][:1])), name
    assert e.feat_explain_new(Fd, rows[:0], rows[:0], 5, ncols, maps=True)["map"].shape == (0, ncols)
    # against the score block: the bf16 rounding of [E|Bp] there, bounded by 2^-8 x the sum of the absolute terms
    blk = e.score_new_block(0, U, e.project_rows(Fd)).cpu().numpy()[grouped, rows]
    Fa = np.abs(F[rows].astype(np.float64))
    scale = ((np.abs(t["Tu"][grouped].astype(np.float64)) @ np.abs(t["E"].astype(np.float64)).T) * Fa).sum(1) + \
        Fa @ np.abs(t["Bp"].astype(np.float64))
    bound = (1e-5 if dtype == "fp32" else 2.0 ** -8) * scale + 1e-6
    print("expl %s: |score - score_new_block| max %.3e, bound min %.3e" % (dtype, np.abs(g["score"] - blk).max(), bound.min()))
    assert (np.abs(g["score"].astype(np.float64) - blk) <= bound).all()
    e.sync_check()
    e.close()


# ---- GradFashion -------------------------------------------------------------------------------------------------------------
def _gf_visual(p, Fc, Fe, dtype):
    """gradfashion_ref's visual term for new rows: Tu.(vf E) + vf.Bp, vf = [Fc Ec | Fe Ee] (GradFashionRef.call / predict_all)."""
    c = lambda x: torch.as_tensor(np.asarray(x)).to(dtype) if not isinstance(x, torch.Tensor) else x.to(dtype)
    vf = torch.cat([c(Fc) @ c(p["Ec"]), c(Fe) @ c(p["Ee"])], 1)
    return (c(p["Tu"]) @ (vf @ c(p["E"])).T + (vf @ c(p["Bp"]).reshape(-1))[None, :]).numpy()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_factored_handle_after_adam_steps(dtype):
    t, F = _gf_setup(dtype)
    e = _gf_engine(t, F, dtype, optimizer="adam_tf23", lr=2e-3, reg=1e-3)
    rs = np.random.RandomState(45)
    for _ in range(3):
        e.step(*(torch.as_tensor(rs.randint(m, size=64).astype(np.int32), device="cuda") for m in (300, 600, 600)))
    n = 200
    Fn = _new_rows(n, PAD[dtype], Dc + De, dtype, seed=46)
    got = e.score_new_block(0, 300, e.project_rows(Fn)).cpu().numpy()
    ref = GradFashionRef(t, reg=1e-3).load(e.t, 3)
    Fc, Fe = Fn[:, :Dc], Fn[:, Dc:Dc + De]
    v64, v32 = _gf_visual(ref.p, Fc, Fe, torch.float64), _gf_visual(ref.p, Fc, Fe, torch.float32)
    E, Bp = ref.effective()
    np.testing.assert_allclose(e.t["E_eff"][:Dc + De].cpu().numpy(), E.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(e.t["Bp_eff"][:Dc + De].cpu().numpy(), Bp.numpy(), rtol=1e-5, atol=1e-6)
    if dtype == "fp32":
        gdev, allow = _report("factored fp32 (gradfashion_ref visual term)", v64, v32, got)
        assert gdev <= allow
    else:
        r64, r32 = (N.scores(e.t["Tu"], Fn, e.t["E_eff"], e.t["Bp_eff"], 0, 300, dtype, dt) for dt in (torch.float64, torch.float32))
        gdev, allow = _report("factored bf16 (the handle's E_eff, bf16-rounded)", r64, r32, got)
        assert gdev <= allow
        Fa = np.abs(Fn[:, :Dc + De].astype(np.float64))
        scale = np.abs(ref.p["Tu"].numpy()) @ (Fa @ np.abs(E.numpy())).T + (Fa @ np.abs(Bp.numpy()))[None, :]
        print("factored bf16: |score - gradfashion_ref visual term| max %.3e, bound min %.3e" % (
            np.abs(got - v64).max(), (2.0 ** -8 * scale + 1e-6).min()))
        assert (np.abs(got - v64) <= 2.0 ** -8 * scale + 1e-6).all()
    e.sync_check()
    e.close()


def test_factored_model_prepares_colour_and_edge_rows():
    from fashionvisualexpl_recommend_amd.models import GradFashion
    from test_gpu_gradfashion import _data, _params
    U, I = 200, 300
    rs = np.random.RandomState(47)
    Fc, Fe = rs.rand(I, 10) * 9.0, synth.make_features(I, 21, seed=48)
    p = _params(optimizer="sgd")
    m = GradFashion(_data(U, I, p), p, features=(Fc, Fe))
    Fd = m.prepare_new_items((Fc[[4, 8]], Fe[[4, 8]]))
    assert tuple(Fd.shape) == (2, 32) and torch.equal(Fd.view(torch.int32), m.engine._t["F"][[4, 8]].view(torch.int32))
    assert m.score_new_items((Fc[:7] * 2, Fe[:7])).shape == (U, 7)
    for bad in ((Fc[:3], Fe[:2]), (Fc[:3, :9], Fe[:3]), Fc[:3]):
        with pytest.raises(ValueError):
            m.prepare_new_items(bad)
    sd = m.state_dict()
    assert float(sd["color_norm"]) == float(np.abs(Fc).max()) and float(sd["edge_norm"]) == float(np.abs(Fe).max())
    m.load_state_dict({n: v for n, v in sd.items() if n not in ("color_norm", "edge_norm")})
    assert float(m.color_norm) == float(np.abs(Fc).max())
    m.engine.close()


# ---- neutrality and lifecycle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,form", [("sgd", None), ("adam_tf23", "lazy"), ("adam_tf23", "sweep")])
def test_the_calls_leave_the_state_alone(monkeypatch, opt, form):
    """Tables and Adam slots are bit-identical before and after the three calls, and a 6-step run with them between steps 3 and 4
    ends bit-identical to a run without them (duplicate-free batches: the step itself is then free of atomic-order noise)."""
    t = _tables(300, 600, 16, 12, 128, 100, "bf16", seed=17)
    batches = _unique_batches(300, 600, 64, 6, seed=18)
    F = _new_rows(77, 128, 100, "bf16", seed=49)
    rs = np.random.RandomState(50)
    u, r = rs.randint(300, size=500), rs.randint(77, size=500)
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
                e.score_new_block(0, 300, e.project_rows(F))
                e.feat_explain_new(F, u, r, 5, 100, maps=True)
                torch.cuda.synchronize()
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
    lib = _ffi.lib()
    gc.collect()
    live = lib.bprx_live_device_allocs()
    t = _tables(50, 80, 16, 12, 256, 200, "bf16", seed=51)
    e = _vbpr(t, "bf16")
    f8 = _vbpr(t, "fp8")
    m = Engine(model="bprmf", num_users=50, num_items=80, embed_k=16, optimizer="sgd", lr=0.05, reg=0.0, max_batch=64)
    m.bind(t["Gu"], t["Gi"], t["Bi"])
    unbound = Engine(model="vbpr", num_users=50, num_items=80, embed_k=16, embed_d=12, feat_dim=256, feat_dtype="bf16", optimizer="sgd",
                     max_batch=64)
    held = lib.bprx_live_device_allocs()
    F = _new_rows(40, 256, 200, "bf16", seed=52)
    Fd = _dev(e, F)
    u, r = np.arange(40, dtype=np.int32), np.arange(40, dtype=np.int32)[::-1].copy()
    P = e.project_rows(Fd)
    S = e.score_new_block(0, 50, P)
    good = _explain(e, Fd, u, r, 5, 200, True)
    e.topk_rows(S, 5)
    assert lib.bprx_live_device_allocs() == held                    # the calls allocated nothing

    def usable():
        assert _same(good, _explain(e, Fd, u, r, 5, 200, True))
        assert np.array_equal(_bits(P.cpu().numpy()), _bits(e.project_rows(Fd).cpu().numpy()))
        e.sync_check()

    for eng, code in ((f8, _ffi.E_INVALID), (m, _ffi.E_INVALID), (unbound, _ffi.E_STATE)):
        for call in (lambda: eng.project_rows(F), lambda: eng.score_new_block(0, 50, P), lambda: eng.topk_rows(S, 5),
                     lambda: eng.feat_explain_new(F, u, r, 5, 200)):
            with pytest.raises(_ffi.BprxError) as err:
                call()
            assert err.value.code == code
    assert "fp8" in lib.bprx_last_error(f8.h).decode()
    assert lib.bprx_proj_stride(m.h) < 0 and lib.bprx_proj_stride(f8.h) == 16
    assert f8.score_block(0, 50).shape == (50, 80)                  # the fp8 handle goes on scoring its catalogue
    f8.sync_check()
    assert m.score_pairs(u, u).shape == (40,)
    for kw in (dict(top=0), dict(top=33), dict(ncols=0), dict(ncols=257)):
        with pytest.raises(_ffi.BprxError) as err:
            e.feat_explain_new(Fd, u, r, **dict(dict(top=5, ncols=200), **kw))
        assert err.value.code == _ffi.E_INVALID, kw
    for K in (0, 1025):
        with pytest.raises(_ffi.BprxError) as err:
            e.topk_rows(S, K)
        assert err.value.code == _ffi.E_INVALID
    p = lambda x: x.data_ptr()
    assert lib.bprx_project_rows(e.h, p(Fd), -1, p(P), None) == _ffi.E_INVALID
    assert lib.bprx_project_rows(e.h, p(Fd), 1 << 31, p(P), None) == _ffi.E_INVALID
    assert lib.bprx_project_rows(e.h, None, 40, p(P), None) == _ffi.E_INVALID
    assert lib.bprx_project_rows(e.h, None, 0, None, None) == 0
    assert lib.bprx_score_new_block(e.h, 0, 51, p(P), 40, p(S), None) == _ffi.E_INVALID
    with pytest.raises(ValueError):
        e.project_rows(F[:, :128])
    usable()
    # row = n_new and user = U: clamped, and reported by sync_check (once)
    g = _explain(e, Fd, np.array([50, 1], np.int32), np.array([40, 2], np.int32), 5, 200, True)
    with pytest.raises(_ffi.BprxError) as err:
        e.sync_check()
    assert err.value.code == _ffi.E_RANGE
    assert _same(g, _explain(e, Fd, np.array([49, 1], np.int32), np.array([39, 2], np.int32), 5, 200, True))
    usable()
    assert lib.bprx_live_device_allocs() == held
    for eng in (e, f8, m, unbound):
        eng.close()
    assert lib.bprx_live_device_allocs() == live


# ---- files -------------------------------------------------------------------------------------------------------------------
def _cli_dataset(tmp_path, rec):
    U, I = 30, 60
    tr, va, te = synth.make_interactions(U, I, per_user=8, seed=53)
    rs = np.random.RandomState(54)
    if rec == "vbpr":
        synth.write_dataset(str(tmp_path), "toy", tr, va, te, I, features=synth.make_features(I, 128, seed=55))
        np.save(str(tmp_path / "new.npy"), synth.make_features(7, 128, seed=56) * 2.0)
        return [str(tmp_path / "new.npy")], 7, 128
    synth.write_dataset(str(tmp_path), "toy", tr, va, te, I)
    synth.write_grad_fashion_features(str(tmp_path), "toy", rs.rand(I, 10), synth.make_features(I, 21, seed=57))
    np.save(str(tmp_path / "new_c.npy"), rs.rand(40, 10))
    np.save(str(tmp_path / "new_e.npy"), synth.make_features(40, 21, seed=58))
    return [str(tmp_path / "new_c.npy"), str(tmp_path / "new_e.npy")], 40, 31


@pytest.mark.parametrize("rec,dtype", [("vbpr", "bf16"), ("grad_fashion", "fp32")])
def test_cli_writes_new_item_files_next_to_unchanged_recommendations(tmp_path, rec, dtype):
    from fashionvisualexpl_recommend_amd import train_rec
    paths, n_new, ncols = _cli_dataset(tmp_path, rec)
    U, top_k = 30, 10
    # --batch_size 1: a step adds at most one term to a gradient row, so runs of the same seed agree bit for bit
    common = ["--rec", rec, "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--embed_color", "4", "--embed_edges", "6", "--reg", "0.01", "--top_k", str(top_k), "--lr", "0.01",
              "--dtype", dtype]
    res = [str(tmp_path / ("res%d" % q)) for q in range(3)]
    train_rec.train(common + ["--results_root", res[0]])
    train_rec.train(common + ["--results_root", res[1], "--new_items"] + paths)
    train_rec.train(common + ["--results_root", res[2], "--feat_explain", "3", "--new_items"] + paths)
    rdir = [os.path.join(r, "rec_results", "toy", rec) for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] if "new-" in f]
    assert [f for f in files[1] if "new-" not in f] == files[0]
    assert [f for f in files[2] if "new-" not in f and "expl-" not in f] == files[0]
    base = [f for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(base) == 2
    for f in base:                                                   # the catalogue's files: the bytes of the run without the flag
        for q in (1, 2):
            assert open(os.path.join(rdir[0], f), "rb").read() == open(os.path.join(rdir[q], f), "rb").read(), (f, q)
        new = f.replace("recs-", "new-recs-", 1)
        expl = f.replace("recs-", "new-expl-", 1)
        assert new in files[1] and new in files[2] and expl in files[2] and expl not in files[1]
        assert open(os.path.join(rdir[1], new), "rb").read() == open(os.path.join(rdir[2], new), "rb").read()
        rrows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[2], new))]
        kk = min(top_k, n_new)
        assert len(rrows) == U * kk and all(len(r) == 3 for r in rrows)
        assert [int(r[0]) for r in rrows] == [u for u in range(U) for _ in range(kk)]
        assert all(0 <= int(r[1]) < n_new for r in rrows)
        for u in range(U):
            sc = [float(r[2]) for r in rrows[u * kk:(u + 1) * kk]]
            assert sc == sorted(sc, reverse=True) and len({r[1] for r in rrows[u * kk:(u + 1) * kk]}) == kk
        erows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[2], expl))]
        L = min(3, ncols)
        assert all(len(r) == 6 for r in erows) and len(erows) == L * len(rrows)
        pairs = {(r[0], r[1]) for r in rrows}
        for q, rr in enumerate(rrows):
            blk = erows[L * q:L * q + L]
            assert all((b[0], b[1]) in pairs for b in blk)
            assert [(b[0], b[1], int(b[3])) for b in blk] == [(rr[0], rr[1], s) for s in range(L)]
            assert all(0 <= int(b[4]) < ncols for b in blk) and len({b[2] for b in blk}) == 1
            c = [float(b[5]) for b in blk]
            assert c == sorted(c, reverse=True)
    assert any(f.startswith("best-new-recs-") for f in files[1]) and any(f.startswith("best-new-expl-") for f in files[2])
