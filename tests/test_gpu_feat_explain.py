"""bprx_feat_explain on the MI355X against its float64 restatement (tests/feat_explain_ref.py).

Allowance per output (score, base, visual, contrib, map): 32 x the max-abs deviation of the FLOAT32 restatement from the float64
one over the pairs of the case, never below one float32 ulp of the output's largest magnitude.  One sample of float32 rounding is
what the restatement gives; the factor 32 covers the kernel's other summation order and its fused multiply-adds.  Every check
prints its triples (float32 deviation / allowance / GPU deviation).  Nothing is compared across precisions by identity, so no
near-tie has to be excluded: a returned contribution is held against the float64 contribution AT THE RETURNED COLUMN and against
the r-th largest float64 contribution.  What is exact is checked exactly: the list against the GPU's own map, score == base +
visual, two calls, with and without the map.

The tiny case's n = 1 call is the first pair of its n = 5 call, and the allowance of both comes from those five pairs (the pairs
of the case): the max over five samples, not one sample's luck."""
import gc
import os

import numpy as np
import pytest
import torch

import feat_explain_ref as X
from fashionvisualexpl_recommend_amd import _ffi, synth
from gradfashion_ref import GradFashionRef
from oracle import oracle as orc
from test_gpu_gradfashion import Dc, De, _engine as _gf_engine, _score_bound, _setup as _gf_setup

pytestmark = pytest.mark.gpu

OUTPUTS = ("score", "base", "visual", "contrib", "map")


def _tables(U, I, k, d, D, ncols, dtype, seed=0, zero_frac=None):
    """VBPR tables; F has `ncols` real columns and zero padding up to D, and holds values its dtype represents exactly."""
    rs = np.random.RandomState(seed)
    F = np.zeros((I, D), np.float32)
    f = synth.make_features(I, ncols, seed=seed)
    if zero_frac is not None:
        f = np.abs(rs.standard_normal((I, ncols))).astype(np.float32) * (rs.random_sample((I, ncols)) >= zero_frac)
    F[:, :ncols] = f / np.abs(f).max()
    if dtype == "bf16":
        F = orc.bf16_round(F)
    return dict(Gu=synth.glorot_uniform(rs, U, k), Gi=synth.glorot_uniform(rs, I, k), Bi=rs.uniform(-1, 1, I).astype(np.float32),
                Tu=synth.glorot_uniform(rs, U, d), F=F, E=synth.glorot_uniform(rs, D, d),
                Bp=synth.glorot_uniform(rs, D, 1).reshape(-1))


def _vbpr(t, dtype, optimizer="sgd", B=256, **kw):
    from fashionvisualexpl_recommend_amd.engine import Engine
    U, k = t["Gu"].shape
    I, (D, d) = t["Gi"].shape[0], t["E"].shape
    return Engine(model="vbpr", num_users=U, num_items=I, embed_k=k, embed_d=d, feat_dim=D, feat_dtype=dtype, optimizer=optimizer,
                  lr=0.05, reg=1e-3, max_batch=B, **kw).bind(**t)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[n]), _bits(b[n])) for n in a if n in b) and (set(a) - {"map"}) == (set(b) - {"map"})


def _call(e, u, i, top, ncols, maps):
    return {n: v.cpu().numpy() for n, v in e.feat_explain(u, i, top, ncols, maps=maps).items()}


def _allowances(r64, r32, top):
    """{output: (float32 deviation, allowance)} over the pairs of r64 / r32 (restatements of the same pairs)."""
    kk = min(top, r64["map"].shape[1])
    s64 = -np.sort(-r64["map"], axis=1, kind="stable")[:, :kk]
    s32 = -np.sort(-r32["map"].astype(np.float64), axis=1, kind="stable")[:, :kk]
    out = {}
    for n in OUTPUTS:
        a, b = (s64, s32) if n == "contrib" else (r64[n], r32[n].astype(np.float64))
        dev = float(np.abs(a - b).max())
        out[n] = (dev, max(32.0 * dev, float(np.spacing(np.float32(np.abs(a).max())))))
    return out


def _check(e, tables, u, i, ncols, top, tag, pool=None):
    """One call with the map (and one without, and a second one): every property of the module docstring.  `pool`: the pairs
    (users, items) the allowances are taken over, when they are more than the call's own."""
    u, i = np.asarray(u, np.int32), np.asarray(i, np.int32)
    n = len(u)
    got = _call(e, u, i, top, ncols, True)
    assert _same_bits(got, _call(e, u, i, top, ncols, True)), tag + ": two calls differ"
    assert _same_bits(got, _call(e, u, i, top, ncols, False)), tag + ": the call without the map differs"
    e.sync_check()
    assert got["map"].shape == (n, ncols) and got["col"].shape == (n, top) and got["col"].dtype == np.int32
    r64 = X.feat_explain_ref(tables, u, i, ncols)
    pu, pi = (u, i) if pool is None else pool
    allow = _allowances(r64 if pool is None else X.feat_explain_ref(tables, pu, pi, ncols),
                        X.feat_explain_ref(tables, pu, pi, ncols, torch.float32), top)
    kk = min(top, ncols)
    s64 = -np.sort(-r64["map"], axis=1, kind="stable")[:, :kk]
    rows = np.arange(n)[:, None]
    col, con = got["col"][:, :kk], got["contrib"][:, :kk]
    assert (col >= 0).all() and (col < ncols).all()
    dev = {"score": np.abs(got["score"] - r64["score"]), "base": np.abs(got["base"] - r64["base"]),
           "visual": np.abs(got["visual"] - r64["visual"]), "map": np.abs(got["map"] - r64["map"]),
           "contrib": np.maximum(np.abs(con - r64["map"][rows, col]), np.abs(con - s64))}
    for name in OUTPUTS:
        print("%s %s: float32 deviation %.3e / allowance %.3e / GPU deviation %.3e" % (tag, name, allow[name][0], allow[name][1],
                                                                                          float(dev[name].max())))
    for name in OUTPUTS:
        assert float(dev[name].max()) <= allow[name][1], (tag, name, float(dev[name].max()), allow[name])
    # the list: non-increasing, ascending columns among equal values, the slots beyond ncols empty
    assert (con[:, :-1] >= con[:, 1:]).all()
    eq = con[:, :-1] == con[:, 1:]
    assert (col[:, :-1][eq] < col[:, 1:][eq]).all()
    assert (got["col"][:, kk:] == -1).all() and not _bits(got["contrib"][:, kk:]).any()
    # exact self-consistency
    assert np.array_equal(_bits(con), _bits(got["map"][rows, col]))
    order = np.argsort(-got["map"], axis=1, kind="stable")[:, :kk]
    assert np.array_equal(order, col), tag + ": the list is not the stable descending sort of the map"
    assert np.array_equal(_bits(got["score"]), _bits(got["base"] + got["visual"]))
    return got, r64


def _vbpr_score_bound(t, u, i, dtype):
    """_score_bound of tests/test_gpu_gradfashion.py for plain VBPR tables: a rounding unit of the operands times the sum of the
    absolute terms of each score, + 1e-6."""
    T = X.as_tables(t)
    u, i = torch.as_tensor(u).long(), torch.as_tensor(i).long()
    Fi = T["F"][i].abs()
    vis = ((T["Tu"][u].abs() @ T["E"].abs().T) * Fi).sum(1) + Fi @ T["Bp"].abs()
    scale = T["Bi"][i].abs() + (T["Gu"][u] * T["Gi"][i]).abs().sum(1) + vis
    return (1e-5 if dtype == "fp32" else 2.0 ** -8) * scale.numpy() + 1e-6


def _orders(U, I, n, seed):
    """(users, items) in three orders: grouped by user in runs of 20, shuffled, one user for all n."""
    rs = np.random.RandomState(seed)
    grouped = np.repeat(rs.randint(U, size=n // 20), 20).astype(np.int32)
    items = rs.randint(I, size=n).astype(np.int32)
    perm = rs.permutation(n)
    return {"grouped": (grouped, items), "shuffled": (grouped[perm], items[perm]), "one_user": (np.full(n, 17, np.int32), items),
            "perm": perm}


BASE = {"fp32": 400, "bf16": 512}
_cache = {}


def _base(dtype):
    if dtype not in _cache:
        t = _tables(300, 600, 16, 12, BASE[dtype], 390, dtype, seed=1)
        _cache[dtype] = (t, _vbpr(t, dtype))
    return _cache[dtype]


@pytest.mark.parametrize("order", ["grouped", "shuffled", "one_user"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_base_case_three_orders_and_the_model_score(dtype, order):
    t, e = _base(dtype)
    u, i = _orders(300, 600, 1000, seed=2)[order]
    for top in (1, 5, 32):
        got, _ = _check(e, t, u, i, 390, top, "base %s %s top %d" % (dtype, order, top))
    model = e.score_pairs(u, i).cpu().numpy()
    bound = _vbpr_score_bound(t, u, i, dtype)
    print("base %s %s: |score - score_pairs| max %.3e, bound min %.3e" % (dtype, order, np.abs(got["score"] - model).max(), bound.min()))
    assert (np.abs(got["score"].astype(np.float64) - model) <= bound).all()


def test_orders_agree_pair_by_pair():
    """A pair's outputs depend on the pair alone: the shuffled call returns the grouped call's rows, bit for bit."""
    t, e = _base("bf16")
    o = _orders(300, 600, 1000, seed=2)
    perm = o["perm"]
    grouped, shuffled = _call(e, *o["grouped"], 5, 390, True), _call(e, *o["shuffled"], 5, 390, True)
    for name in grouped:
        assert np.array_equal(_bits(shuffled[name]), _bits(grouped[name][perm])), name


def test_tiny_calls():
    t, e = _base("fp32")
    rs = np.random.RandomState(3)
    u5, i5 = rs.randint(300, size=5).astype(np.int32), rs.randint(600, size=5).astype(np.int32)
    g5, _ = _check(e, t, u5, i5, 390, 5, "tiny n=5")
    g1, _ = _check(e, t, u5[:1], i5[:1], 390, 5, "tiny n=1", pool=(u5, i5))
    for name in g1:
        assert np.array_equal(_bits(g1[name]), _bits(g5[name][:1])), name
    empty = e.feat_explain(u5[:0], i5[:0], 5, 390, maps=True)
    assert empty["score"].shape == (0,) and empty["col"].shape == (0, 5) and empty["map"].shape == (0, 390)
    e.sync_check()
    u, i = rs.randint(300, size=40), rs.randint(600, size=40)
    got, _ = _check(e, t, u, i, 20, 32, "tiny ncols=20 top=32")       # slots 20..31 are -1 / 0.0f
    assert (got["col"][:, 20:] == -1).all() and (got["col"][:, :20] >= 0).all()


@pytest.mark.parametrize("D,d", [(68, 12), (65, 7)])
@pytest.mark.parametrize("ncols", [64, 65])
def test_tiny_column_step_edges(D, d, ncols):
    """ncols 64 and 65 (one column step and one column more), with rows of 16-byte multiples (D 68: vector loads of F, E and the
    map where ncols allows) and without (D 65, d 7: the scalar forms)."""
    t = _tables(50, 70, 16, d, D, ncols, "fp32", seed=4)
    e = _vbpr(t, "fp32")
    rs = np.random.RandomState(5)
    u, i = np.sort(rs.randint(50, size=70)), rs.randint(70, size=70)
    for top in (1, 32):
        _check(e, t, u, i, ncols, top, "tiny D=%d d=%d ncols=%d top %d" % (D, d, ncols, top))
    e.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wide_rows(dtype):
    """feat_dim = ncols = 4096, d = k = 64: 64 column steps (fp32; 8 chunks of 512 columns in bf16), 16 KB of w."""
    t = _tables(40, 300, 64, 64, 4096, 4096, dtype, seed=6)
    e = _vbpr(t, dtype)
    rs = np.random.RandomState(7)
    u, i = np.repeat(rs.randint(40, size=32), 8), rs.randint(300, size=256)
    got, _ = _check(e, t, u, i, 4096, 32, "wide %s" % dtype)
    model = e.score_pairs(u, i).cpu().numpy()
    assert (np.abs(got["score"].astype(np.float64) - model) <= _vbpr_score_bound(t, u, i, dtype)).all()
    e.close()


def test_fp8_features():
    """feat_dim 256, ncols 200; the features are quantised as Engine.bind does and the restatement gets codes.float() / feat_scale.
    The codes cover subnormals (|f| 448 < 2^-6) and the top of the range (448)."""
    t = _tables(60, 200, 16, 12, 256, 200, "fp32", seed=8)
    t["F"][:, :200] *= np.random.RandomState(9).choice([1.0, 1e-2, 3e-5], size=(200, 200)).astype(np.float32)
    t["F"][0, 0] = 1.0
    e = _vbpr(t, "fp8")
    codes = e.t["F"]
    assert codes.dtype == torch.float8_e4m3fn
    raw = codes.view(torch.uint8).cpu().numpy()
    assert ((raw & 0x78) == 0).any() and ((raw & 0x7f) > 0)[(raw & 0x78) == 0].any() and (raw == 0x7e).any()
    tt = dict(t, F=(codes.float() / e.feat_scale).cpu().numpy())
    rs = np.random.RandomState(10)
    u, i = np.sort(rs.randint(60, size=300)), rs.randint(200, size=300)
    for top in (5, 32):
        _check(e, tt, u, i, 200, top, "fp8 top %d" % top)
    e.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_factored_model(dtype):
    """GradFashion (the _setup shape of tests/test_gpu_gradfashion.py): the handle's own E_eff / Bp_eff are the tables of the
    restatement; the colour and the edge columns of the map sum to bprx_explain_pairs."""
    t, F = _gf_setup(dtype)
    e = _gf_engine(t, F, dtype)
    rs = np.random.RandomState(11)
    for _ in range(3):                                              # away from the initial tables
        e.step(*(torch.as_tensor(rs.randint(m, size=64).astype(np.int32), device="cuda") for m in (300, 600, 600)))
    tt = dict(Gu=e.t["Gu"], Gi=e.t["Gi"], Bi=e.t["Bi"], Tu=e.t["Tu"], E=e.t["E_eff"], Bp=e.t["Bp_eff"], F=e.t["F"].float())
    u, i = np.sort(rs.randint(300, size=400)), rs.randint(600, size=400)
    got, _ = _check(e, tt, u, i, Dc + De, 5, "factored %s" % dtype)
    ref = GradFashionRef(t, reg=0.1).load(e.t, 0)
    bound = _score_bound(ref, u, i, "fp32")
    parts = e.explain_pairs(u, i).cpu().numpy().astype(np.float64)
    m = got["map"].astype(np.float64)
    assert (np.abs(m[:, :Dc].sum(1) - parts[:, 0]) <= bound).all() and (np.abs(m[:, Dc:].sum(1) - parts[:, 1]) <= bound).all()
    model = e.score_pairs(u, i).cpu().numpy()
    assert (np.abs(got["score"].astype(np.float64) - model) <= _score_bound(ref, u, i, dtype)).all()
    e.close()


def test_equal_columns_tie_and_rank_in_column_order():
    """Columns 7 and 19 of F equal in every row, E[7] == E[19], Bp[7] == Bp[19]: bit-equal contributions, 7 ranked right before 19."""
    t = _tables(50, 80, 16, 12, 48, 40, "fp32", seed=12)
    t["F"][:, 7] = t["F"][:, 19] = np.abs(np.random.RandomState(13).standard_normal(80)).astype(np.float32) + 0.5
    t["E"][19], t["Bp"][19] = t["E"][7], t["Bp"][7]
    e = _vbpr(t, "fp32")
    rs = np.random.RandomState(14)
    u, i = rs.randint(50, size=200), rs.randint(80, size=200)
    got, _ = _check(e, t, u, i, 40, 32, "ties")
    assert np.array_equal(_bits(got["map"][:, 7]), _bits(got["map"][:, 19]))
    r7, c7 = np.nonzero(got["col"][:, :-1] == 7)
    assert len(r7) > 100 and (got["col"][r7, c7 + 1] == 19).all()
    r19, c19 = np.nonzero(got["col"] == 19)
    assert (c19 > 0).all() and (got["col"][r19, c19 - 1] == 7).all()
    e.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_zero_contributions_rank_in_column_order_whatever_their_sign(dtype):
    """A relu-like F with 85 % exact zeros: most contributions are 0 * w = +-0.0 and fill the list behind the few positive ones."""
    D = 256
    t = _tables(50, 120, 16, 12, D, 200, dtype, seed=15, zero_frac=0.85)
    assert (t["F"][:, :200] == 0).mean() >= 0.7
    e = _vbpr(t, dtype)
    rs = np.random.RandomState(16)
    u, i = np.sort(rs.randint(50, size=300)), rs.randint(120, size=300)
    got, _ = _check(e, t, u, i, 200, 32, "zeros %s" % dtype)
    z = got["contrib"] == 0
    assert z.sum() > 1000
    sign = np.signbit(got["contrib"][z])
    assert sign.any() and not sign.all()                             # both +0.0 and -0.0 are in the lists
    both = z[:, :-1] & z[:, 1:]
    assert (got["col"][:, :-1][both] < got["col"][:, 1:][both]).all()
    e.close()


def _snapshot(e):
    return {n: v.detach().clone() for n, v in e._t.items() if n != "F"}


def _unique_batches(U, I, B, steps, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        it = rs.choice(I, 2 * B, replace=False)
        out.append(tuple(torch.as_tensor(x.astype(np.int32), device="cuda") for x in (rs.choice(U, B, replace=False), it[:B], it[B:])))
    return out


@pytest.mark.parametrize("opt,form", [("sgd", None), ("adam_tf23", "lazy"), ("adam_tf23", "sweep")])
def test_the_call_leaves_the_state_alone(monkeypatch, opt, form):
    """Tables and Adam slots are bit-identical before and after a call, and a 6-step run with a call between steps 3 and 4 ends
    bit-identical to a run without it (duplicate-free batches: the step itself is then free of atomic-order noise)."""
    t = _tables(300, 600, 16, 12, 128, 100, "bf16", seed=17)
    batches = _unique_batches(300, 600, 64, 6, seed=18)
    rs = np.random.RandomState(19)
    u, i = rs.randint(300, size=500), rs.randint(600, size=500)
    end = []
    if form is not None:
        monkeypatch.setenv("BPRX_ADAM_LAZY", "1" if form == "lazy" else "0")      # (the variable overrides the engine's own choice)
    for with_call in (False, True):
        e = _vbpr(t, "bf16", optimizer=opt, B=64)
        if form is not None:
            assert e.adam_is_lazy() == (form == "lazy")
        for s, b in enumerate(batches):
            if s == 3 and with_call:
                e.sync_adam()                                        # a lazy handle has nothing pending at the first snapshot
                before = _snapshot(e)
                e.feat_explain(u, i, 5, 100, maps=True)
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
    gc.collect()                                                    # engines other tests dropped without closing go now, not later
    live = lib.bprx_live_device_allocs()
    t = _tables(50, 80, 16, 12, 48, 40, "fp32", seed=20)
    e = _vbpr(t, "fp32")
    m = Engine(model="bprmf", num_users=50, num_items=80, embed_k=16, optimizer="sgd", lr=0.05, reg=0.0, max_batch=64)
    m.bind(t["Gu"], t["Gi"], t["Bi"])
    held = lib.bprx_live_device_allocs()
    u, i = np.arange(40, dtype=np.int32), np.arange(40, dtype=np.int32)
    good = _call(e, u, i, 5, 40, True)

    def usable():
        assert _same_bits(good, _call(e, u, i, 5, 40, True))
        e.sync_check()

    for kw in (dict(top=0), dict(top=33), dict(ncols=0), dict(ncols=49)):
        with pytest.raises(_ffi.BprxError) as err:
            e.feat_explain(u, i, **dict(dict(top=5, ncols=40), **kw))
        assert err.value.code == _ffi.E_INVALID, kw
        usable()
    with pytest.raises(ValueError):
        e.feat_explain(u, i[:3])
    ud, idv = torch.as_tensor(u, device="cuda"), torch.as_tensor(i, device="cuda")
    out = {n: v for n, v in e.feat_explain(u, i, 5, 40).items()}
    p = lambda x: x.data_ptr()
    rc = lib.bprx_feat_explain(e.h, p(e.t["F"]), p(ud), p(idv), 40, 40, 5, p(out["score"]), p(out["base"]), None, p(out["col"]),
                               p(out["contrib"]), None, None)
    assert rc == _ffi.E_INVALID                                     # a null output pointer
    usable()
    with pytest.raises(_ffi.BprxError) as err:
        m.feat_explain(u, i, 5, 40)
    assert err.value.code == _ffi.E_INVALID                        # (a handle of the wrong kind, as everywhere)
    assert m.score_pairs(u, i).shape == (40,)
    m.sync_check()
    for bad_u, bad_i in ((50, 3), (3, 80), (-1, 3)):                 # clamped, and reported by sync_check
        g = _call(e, np.array([bad_u, 1], np.int32), np.array([bad_i, 2], np.int32), 5, 40, True)
        with pytest.raises(_ffi.BprxError) as err:
            e.sync_check()
        assert err.value.code == _ffi.E_RANGE
        cu, ci = min(max(bad_u, 0), 49), min(max(bad_i, 0), 79)
        want = _call(e, np.array([cu, 1], np.int32), np.array([ci, 2], np.int32), 5, 40, True)
        assert _same_bits(g, want)
        usable()
    assert lib.bprx_live_device_allocs() == held                    # the calls allocated nothing
    e.close()
    m.close()
    assert lib.bprx_live_device_allocs() == live


# ---- files -----------------------------------------------------------------------------------------------------------------
def _cli_dataset(tmp_path, rec):
    U, I = 30, 60
    tr, va, te = synth.make_interactions(U, I, per_user=8, seed=21)
    if rec == "vbpr":
        synth.write_dataset(str(tmp_path), "toy", tr, va, te, I, features=synth.make_features(I, 40, seed=22))
    else:
        synth.write_dataset(str(tmp_path), "toy", tr, va, te, I)
        synth.write_grad_fashion_features(str(tmp_path), "toy", np.random.RandomState(23).rand(I, 10), synth.make_features(I, 21, seed=24))
    return tr, va, te


@pytest.mark.parametrize("rec", ["vbpr", "grad_fashion"])
def test_cli_writes_explanations_next_to_unchanged_recommendations(tmp_path, rec):
    from fashionvisualexpl_recommend_amd import train_rec
    tr, va, te = _cli_dataset(tmp_path, rec)
    # --batch_size 1: a step adds at most one term to a gradient row, so two runs of the same seed agree bit for bit
    common = ["--rec", rec, "--dataset", "toy", "--data_root", str(tmp_path), "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--embed_d", "8", "--embed_color", "4", "--embed_edges", "6", "--reg", "0.01", "--top_k", "5", "--lr", "0.01"]
    res = [str(tmp_path / "res0"), str(tmp_path / "res1")]
    train_rec.train(common + ["--results_root", res[0]])
    train_rec.train(common + ["--results_root", res[1], "--feat_explain", "3"])
    m = train_rec._last_model
    ncols = 40 if rec == "vbpr" else 31                            # 10 + 21, padded to 32
    assert m.feat_cols == ncols and m.feat_explain == 3
    rdir = [os.path.join(r, "rec_results", "toy", rec) for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] if "expl-" in f]
    assert [f for f in files[1] if "expl-" not in f] == files[0]
    pairs = [(f, f.replace("recs-", "expl-", 1)) for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(pairs) == 2 and all(x in files[1] for _, x in pairs)
    assert "expl-2-%s.tsv" % m.directory_parameters in files[1] and any(f.startswith("best-expl-") for f in files[1])
    for recs, expl in pairs:
        assert open(os.path.join(rdir[0], recs), "rb").read() == open(os.path.join(rdir[1], recs), "rb").read()
        rrows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], recs))]
        erows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], expl))]
        assert all(len(r) == 7 for r in erows) and len(erows) == 3 * len(rrows)
        for q, (u, i) in enumerate((r[0], r[1]) for r in rrows):        # ranks 0, 1, 2 per pair, in the order of the recs rows
            blk = erows[3 * q:3 * q + 3]
            assert [(r[0], r[1], int(r[4])) for r in blk] == [(u, i, s) for s in range(3)]
            assert all(0 <= int(r[5]) < ncols for r in blk) and len({r[2] for r in blk}) == len({r[3] for r in blk}) == 1
            c = [float(r[6]) for r in blk]
            assert c == sorted(c, reverse=True)
    # the model is back at its last state: the rows of expl-2-* are model.explain of the same pairs, value for value
    erows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], "expl-2-%s.tsv" % m.directory_parameters))]
    first = erows[::3]
    ex = m.explain([int(r[0]) for r in first], [int(r[1]) for r in first], top=3)
    f32 = lambda rows, c: np.array([float(r[c]) for r in rows], np.float32)
    assert np.array_equal(_bits(f32(first, 2)), _bits(ex["score"])) and np.array_equal(_bits(f32(first, 3)), _bits(ex["base"]))
    assert np.array_equal(np.array([int(r[5]) for r in erows]).reshape(-1, 3), ex["col"])
    assert np.array_equal(_bits(f32(erows, 6).reshape(-1, 3)), _bits(ex["contrib"]))
    if rec == "vbpr":                                               # the evaluator's host path writes the same expl-* file
        m.evaluator.force_host = True
        m._store_recs(str(tmp_path / "recs-host.tsv"))
        assert open(str(tmp_path / "expl-host.tsv"), "rb").read() == \
            open(os.path.join(rdir[1], "expl-2-%s.tsv" % m.directory_parameters), "rb").read()
        assert [l.split("\t")[:2] for l in open(str(tmp_path / "recs-host.tsv"))] == \
            [l.split("\t")[:2] for l in open(os.path.join(rdir[1], "recs-2-%s.tsv" % m.directory_parameters))]
    else:                                                           # GradFashion: the pairs store_recommendation_grads writes
        want = [(str(u), str(i)) for u in range(30) for i in tr[u] + va[u] + te[u]]
        assert [(r[0], r[1]) for r in first] == want
