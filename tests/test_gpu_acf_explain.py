"""bprx_acf_explain on the MI355X against the float64 restatement (tests/acf_explain_ref.py): test_gpu_acf.py's shape grid, fp32
and bf16 features, histories of 0 .. 3 000 entries with duplicated items, duplicated users and pairs, top 1 / 5 / 32; a caller
CSR other than the bound one; neutrality towards training state in both gradient modes; errors; the CLI's expl-* files.

Allowances: per output, acf_explain_ref.TOL_MULT (32) x the max-abs deviation of the SAME restatement run in float32 on the CPU
from the float64 one, over the pairs of the case (the convention of tests/test_gpu_acf_full.py); every case prints its triples
(float32 deviation / allowance / GPU deviation), the figures of the first GPU run are in DESIGN.md section 9.  The order of
near-equal contributions may hinge on rounding, so identities are never compared across precisions: values are checked at the
positions the GPU returned, and the returned contributions against the SORTED float64 ones."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import acf_explain_ref as X
from acf_ref import ACFRef, random_tables
from fashionvisualexpl_recommend_amd import _ffi, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [  # M, C, k, h, a  (tests/test_gpu_acf.py's grid)
    (1, 200, 16, 64, 64), (9, 512, 128, 64, 64), (49, 512, 16, 32, 48), (49, 2048, 128, 64, 64), (196, 200, 16, 64, 64),
]
LENS = [0, 1, 2, 3000, 5, 40, 7, 1, 0, 3, 17, 2]
INT_FIELDS = ("pos", "hist_item", "peak")
FLOAT_FIELDS = ("alpha", "contrib", "beta_peak")


def _features(rs, I, M, C, dtype):
    F = (np.abs(rs.standard_normal((I, M, C))) * (rs.random_sample((I, M, C)) < 0.5)).astype(np.float32)
    return orc.bf16_round(F) if dtype == "bf16" else F


def _lists(rs, U, I, lens):
    return [sorted(rs.choice(I, n, replace=n > I).tolist()) if n else [] for n in lens]


def _engine(t, F, lists, dtype="fp32", optimizer="sgd", lr=0.05, reg=0.0, B=256, eval_lists=None, gradient=None):
    from fashionvisualexpl_recommend_amd.engine import Engine
    U, k = t["Gu"].shape
    I = t["Gi"].shape[0]
    e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=k, feat_dtype=dtype, optimizer=optimizer, lr=lr, reg=reg,
               max_batch=B)
    kw = {} if gradient is None else {"gradient": gradient}
    return e.bind_acf(t["Gu"], t["Gi"], t["Bi"], F, t["Pi"], {n: t[n] for n in _ffi.ACF_WEIGHTS}, lists, eval_lists, **kw)


def _check(got, r64, allow, users, lists, top, M, tag):
    """Checks 1-4 of the module docstring's plan on one call's outputs (numpy) against the float64 results of the same pairs."""
    g = got
    n = len(users)
    assert g["score"].shape == (n,) and g["base"].shape == (n,)
    for f in INT_FIELDS + FLOAT_FIELDS:
        assert g[f].shape == (n, top), f
    assert g["beta"].shape == (n, top, M)
    dev = {f: 0.0 for f in X.FIELDS}
    for r, u in enumerate(users):
        hist, ref = lists[u], r64[r]
        L = len(hist)
        nv = min(top, L)
        pos = g["pos"][r]
        # 1. structure
        assert ((pos[:nv] >= 0) & (pos[:nv] < L)).all() and len(set(pos[:nv].tolist())) == nv, (tag, r, pos)
        for f in INT_FIELDS:
            assert (g[f][r, nv:] == -1).all(), (tag, r, f)
        for f in FLOAT_FIELDS:
            assert (g[f][r, nv:] == 0.0).all(), (tag, r, f)
        assert (g["beta"][r, nv:] == 0.0).all(), (tag, r)
        assert (g["hist_item"][r, :nv] == np.asarray(hist, np.int64)[pos[:nv]]).all(), (tag, r)
        c = g["contrib"][r, :nv]
        assert (np.diff(c) <= 0).all(), (tag, r, c)
        same = np.diff(c.view(np.int32)) == 0                                  # runs of bit-equal contributions
        assert (np.diff(pos[:nv])[same] > 0).all(), (tag, r, pos, c)
        pk = g["peak"][r, :nv]
        assert ((pk >= 0) & (pk < M)).all(), (tag, r, pk)
        assert (g["beta_peak"][r, :nv] == g["beta"][r, np.arange(nv), pk]).all(), (tag, r)
        # 2. values at the returned positions
        dev["score"] = max(dev["score"], abs(float(g["score"][r]) - float(ref["score"])))
        dev["base"] = max(dev["base"], abs(float(g["base"][r]) - float(ref["base"])))
        if nv:
            p = pos[:nv]
            dev["alpha"] = max(dev["alpha"], float(np.abs(g["alpha"][r, :nv] - ref["alpha"][p]).max()))
            dev["contrib"] = max(dev["contrib"], float(np.abs(c - ref["contrib"][p]).max()))
            dev["beta"] = max(dev["beta"], float(np.abs(g["beta"][r, :nv] - ref["beta"][p]).max()))
            short = ref["beta"][p].max(1) - ref["beta"][p, pk]                 # the peak attains the float64 row's maximum
            assert (short <= allow["beta"]).all(), (tag, r, short.max(), allow["beta"])
            # 3. it is the top: values against the sorted float64 contributions
            want = np.sort(ref["contrib"])[::-1][:nv]
            d3 = float(np.abs(c - want).max())
            assert d3 <= allow["contrib"], (tag, r, "top", d3, allow["contrib"])
        # 4. the whole history returned: the decomposition closes
        if top >= L:
            d4 = abs(float(g["base"][r]) + float(g["contrib"][r].astype(np.float64).sum()) - float(g["score"][r]))
            assert d4 <= allow["score"], (tag, r, "sum", d4, allow["score"])
    for f in X.FIELDS:
        print("%s %-8s fp32 restatement %.3e  allowance %.3e  gpu %.3e" % (tag, f, allow[f] / X.TOL_MULT, allow[f], dev[f]))
    bad = [(f, dev[f], allow[f]) for f in X.FIELDS if not dev[f] <= allow[f]]
    assert not bad, (tag, bad)
    assert dev["score"] <= 1e-5, (tag, dev["score"])                          # test_gpu_acf.py's bound for score_pairs


_CASES = {}


def _grid_case(shape, dtype):
    if (shape, dtype) not in _CASES:
        M, C, k, h, a = shape
        rs = np.random.RandomState(M + C + k)
        U, I = 12, 40
        t = random_tables(rs, U, I, k, C, h, a, scale=10.0)
        F = _features(rs, I, M, C, dtype)
        lists = _lists(rs, U, I, LENS)
        lists[4] = [3, 3, 3, 9, 9]                                       # duplicated history items
        users = list(range(U)) + [3, 5, 5, 4, 4, 0]                     # duplicated users
        items = rs.randint(0, I, len(users)).tolist()
        items[-2] = items[-3]                                            # a duplicated pair (4, i)
        items[U] = items[3]                                              # and one with the long history
        r64 = X.explain_pairs(t, F, users, items, lists, torch.float64)
        r32 = X.explain_pairs(t, F, users, items, lists, torch.float32)
        _CASES.clear()                                                   # one case resident at a time
        _CASES[(shape, dtype)] = (t, F, lists, users, items, r64, X.allowances(r64, r32))
    return _CASES[(shape, dtype)]


@pytest.mark.parametrize("top", [1, 5, 32])
@pytest.mark.parametrize("M,C,k,h,a,dtype", [s + ("fp32",) for s in SHAPES] + [s + ("bf16",) for s in SHAPES if s[1] % 8 == 0])
def test_explain_against_fp64(M, C, k, h, a, dtype, top):
    t, F, lists, users, items, r64, allow = _grid_case((M, C, k, h, a), dtype)
    e = _engine(t, F, lists, dtype)
    out = e.acf_explain(users, items, top=top, maps=True)
    got = {n: v.cpu().numpy() for n, v in out.items()}
    e.sync_check()
    _check(got, r64, allow, users, lists, top, M, "grid/M%d/C%d/k%d/%s/top%d" % (M, C, k, dtype, top))
    x = e.score_pairs(users, items).cpu().numpy().astype(np.float64)
    assert np.abs(got["score"] - x).max() <= 1e-5
    # without maps: the same outputs, no beta; and a second call gives the same bits (fixed summation order, no float atomics)
    again = {n: v.cpu().numpy() for n, v in e.acf_explain(users, items, top=top).items()}
    assert "beta" not in again
    for n in again:
        assert np.array_equal(again[n], got[n]), n
    # duplicated pairs are computed alike
    assert all(np.array_equal(got[n][-2], got[n][-3]) for n in got)
    assert all(np.array_equal(got[n][len(LENS)], got[n][3]) for n in got)


def test_other_histories():
    rs = np.random.RandomState(5)
    U, I, M, C, k = 20, 50, 9, 64, 16
    t = random_tables(rs, U, I, k, C, 64, 64, scale=10.0)
    F = _features(rs, I, M, C, "fp32")
    train = _lists(rs, U, I, rs.randint(0, 12, U))
    other = _lists(rs, U, I, rs.randint(0, 30, U))
    e = _engine(t, F, train)
    users = rs.randint(0, U, 60).tolist()
    items = rs.randint(0, I, 60).tolist()
    r64 = X.explain_pairs(t, F, users, items, other, torch.float64)
    allow = X.allowances(r64, X.explain_pairs(t, F, users, items, other, torch.float32))
    got = {n: v.cpu().numpy() for n, v in e.acf_explain(users, items, top=5, lists=other, maps=True).items()}
    _check(got, r64, allow, users, other, 5, M, "other")
    want = ACFRef(t, F).call(users, items, other).numpy()
    assert np.abs(got["score"] - want).max() <= 1e-5
    got = {n: v.cpu().numpy() for n, v in e.acf_explain(users, items, top=5, csr=e.csr(other), maps=True).items()}
    _check(got, r64, allow, users, other, 5, M, "other/csr")
    # the bound training histories are the default
    r64 = X.explain_pairs(t, F, users, items, train, torch.float64)
    allow = X.allowances(r64, X.explain_pairs(t, F, users, items, train, torch.float32))
    got = {n: v.cpu().numpy() for n, v in e.acf_explain(users, items, top=5, maps=True).items()}
    _check(got, r64, allow, users, train, 5, M, "bound")
    e.sync_check()


def _dev(e, batch):
    return tuple(torch.as_tensor(np.asarray(b), dtype=torch.int32, device=e.device) for b in batch)


def _neutral_inputs(seed=31):
    rs = np.random.RandomState(seed)
    U, I, M, C, k, B = 40, 90, 9, 128, 16, 32
    t = random_tables(rs, U, I, k, C, 64, 64, scale=10.0)
    F = _features(rs, I, M, C, "fp32")
    lists = _lists(rs, U, I, rs.randint(0, 12, U))
    batches = []
    for _ in range(6):                                               # users, pos and neg items all distinct: no two atomic adds meet
        it = rs.permutation(I)[:2 * B]
        batches.append((rs.permutation(U)[:B], it[:B], it[B:]))
    pairs = (rs.randint(0, U, 50).tolist(), rs.randint(0, I, 50).tolist())
    return t, F, lists, batches, pairs


@pytest.mark.parametrize("gradient", ["detached", "full"])
@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
def test_explain_leaves_training_state_alone(gradient, opt):
    t, F, lists, batches, pairs = _neutral_inputs()
    e = _engine(t, F, lists, optimizer=opt, reg=0.05, lr=0.01, gradient=gradient)
    for b in batches[:5]:
        e.step(*_dev(e, b))
    snap = {n: v.clone() for n, v in e.t.items()}                    # tables and Adam slots
    step = e.lib.bprx_get_adam_step(e.h)
    e.acf_explain(*pairs, top=5, maps=True)
    e.acf_explain(*pairs, top=32, lists=[l[::-1] for l in lists])
    e.sync_check()
    assert e.lib.bprx_get_adam_step(e.h) == step and e.acf_gradient() == gradient
    for n, v in snap.items():
        assert torch.equal(e.t[n], v), (gradient, opt, n)


@pytest.mark.parametrize("gradient", ["detached", "full"])
def test_explain_between_steps_does_not_change_the_run(gradient):
    t, F, lists, batches, pairs = _neutral_inputs(37)
    engines = [_engine(t, F, lists, optimizer="adam_tf23", reg=0.05, lr=0.01, gradient=gradient) for _ in range(2)]
    losses = [[], []]
    for s, b in enumerate(batches):
        if s == 3:
            engines[1].acf_explain(*pairs, top=5, maps=True)
        for q, e in enumerate(engines):
            losses[q].append(float(e.step(*_dev(e, b)).item()))
    for e in engines:
        e.sync_check()
    for n in engines[0].t:
        a, b = engines[0].t[n], engines[1].t[n]
        if gradient == "detached":
            assert torch.equal(a, b), n
        else:       # float atomics in arrival order: the bound of test_gpu_acf_full.py's snapshot test for a repeated full run
            assert torch.allclose(a, b, rtol=0, atol=1e-6), n
    if gradient == "detached":
        assert losses[0] == losses[1]


def test_errors_and_handle_stays_usable():
    from fashionvisualexpl_recommend_amd.engine import Engine
    rs = np.random.RandomState(19)
    U, I, M, C, k = 10, 20, 4, 64, 16
    t = random_tables(rs, U, I, k, C, 64, 64)
    F = _features(rs, I, M, C, "fp32")
    lists = _lists(rs, U, I, rs.randint(1, 6, U))
    e = _engine(t, F, lists)
    for top in (0, 33, -1):
        with pytest.raises(_ffi.BprxError) as ex:
            e.acf_explain([1, 2], [3, 4], top=top)
        assert ex.value.code == _ffi.E_INVALID
    plain = Engine(model="bprmf", num_users=8, num_items=9, embed_k=16, optimizer="sgd", lr=0.1, reg=0.0, max_batch=16)
    plain.bind(Gu=synth.glorot_uniform(rs, 8, 16), Gi=synth.glorot_uniform(rs, 9, 16), Bi=np.zeros(9, np.float32))
    with pytest.raises(_ffi.BprxError) as ex:
        plain.acf_explain([1], [2], top=3)
    assert ex.value.code == _ffi.E_STATE
    assert e.acf_explain([], [], top=3)["pos"].shape == (0, 3)       # n = 0 is valid
    bad = [list(l) for l in lists]
    bad[2] = [1, 10 ** 6]                                            # clamped and reported, nothing faults
    e.acf_explain([2], [0], top=3, lists=bad)
    with pytest.raises(_ffi.BprxError) as ex:
        e.sync_check()
    assert ex.value.code == _ffi.E_RANGE
    e.acf_explain([U + 3], [I + 7], top=3)                           # pair indices as well
    with pytest.raises(_ffi.BprxError) as ex:
        e.sync_check()
    assert ex.value.code == _ffi.E_RANGE
    users, items = list(range(U)), rs.randint(0, I, U).tolist()
    r64 = X.explain_pairs(t, F, users, items, lists, torch.float64)
    allow = X.allowances(r64, X.explain_pairs(t, F, users, items, lists, torch.float32))
    got = {n: v.cpu().numpy() for n, v in e.acf_explain(users, items, top=5, maps=True).items()}
    _check(got, r64, allow, users, lists, 5, M, "after-range-error")
    e.sync_check()


def test_model_explain_and_empty_history_rows(tmp_path):
    """models.ACF.explain / explain_ui and the evaluator's files on in-memory lists with two users without any history (the
    dataset loader cannot produce an empty list, so the CLI test below cannot contain that row)."""
    from fashionvisualexpl_recommend_amd import models
    rs = np.random.RandomState(23)
    U, I = 40, 50
    train, val, test = synth.make_interactions(U, I, per_user=8, seed=7)
    for u in (0, 17):
        train[u], val[u] = [], []
    data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=val, test_list=test,
                     params=Namespace(batch_eval=128))
    params = Namespace(epochs=1, batch_size=32, embed_k=16, lr=1e-3, reg=0.05, top_k=5, dataset="toy", rec="acf",
                       layers_component=[32, 1], layers_item=[32, 1], optimizer="adam_tf23", dtype="fp32", acf_explain=3)
    F = np.abs(rs.standard_normal((I, 4, 64))).astype(np.float32)
    m = models.ACF(data, params, features=F)
    ex = m.explain([1, 0, 2], [5, 6, 7], top=4, maps=True)
    assert isinstance(ex["score"], np.ndarray) and ex["beta"].shape == (3, 4, 4) and (ex["pos"][1] == -1).all()
    one = m.explain_ui(1, [5, 9], top=4)
    assert "beta" not in one and np.array_equal(one["contrib"][0], ex["contrib"][0])
    recs, plain, expl = str(tmp_path / "recs.tsv"), str(tmp_path / "plain.tsv"), str(tmp_path / "expl.tsv")
    m.evaluator.store_recommendation(plain)
    m.evaluator.store_recommendation_acf(recs, expl, 3)
    assert open(recs, "rb").read() == open(plain, "rb").read()
    rows = [l.rstrip("\n").split("\t") for l in open(expl)]
    assert all(len(r) == 10 for r in rows)
    for u in (0, 17):
        mine = [r for r in rows if int(r[0]) == u]
        assert len(mine) == 5                                        # one row per recommended item
        for r in mine:
            assert r[4:] == ["-1", "-1", "0.0", "0.0", "-1", "0.0"] and float(r[2]) == float(r[3])
    ev = m.eval_lists()
    for r in rows:
        u, rank, l = int(r[0]), int(r[4]), int(r[5])
        if rank >= 0:
            assert l in ev[u] and 0 <= int(r[8]) < 4


def test_evaluator_host_path_writes_the_same_explanations(tmp_path):
    """store_recommendation falls back to the host for force_host (and for top_k > 1024); store_recommendation_acf follows it:
    the same recs bytes as store_recommendation on that path, and an explanation block for every row."""
    from fashionvisualexpl_recommend_amd import models
    rs = np.random.RandomState(29)
    U, I = 30, 40
    train, val, test = synth.make_interactions(U, I, per_user=8, seed=11)
    data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=val, test_list=test,
                     params=Namespace(batch_eval=16))
    params = Namespace(epochs=1, batch_size=32, embed_k=16, lr=1e-3, reg=0.05, top_k=4, dataset="toy", rec="acf",
                       layers_component=[32, 1], layers_item=[32, 1], optimizer="adam_tf23", dtype="fp32", acf_explain=2)
    m = models.ACF(data, params, features=np.abs(rs.standard_normal((I, 4, 64))).astype(np.float32))
    p = lambda n: str(tmp_path / n)
    m.evaluator.store_recommendation_acf(p("dev_recs"), p("dev_expl"), 2)
    m.evaluator.force_host = True
    m.evaluator.store_recommendation(p("host_plain"))
    m.evaluator.store_recommendation_acf(p("host_recs"), p("host_expl"), 2)
    assert open(p("host_recs"), "rb").read() == open(p("host_plain"), "rb").read()
    rrows = [l.split("\t") for l in open(p("host_recs"))]
    erows = [l.rstrip("\n").split("\t") for l in open(p("host_expl"))]
    assert len(rrows) == U * 4
    assert [(r[0], r[1]) for r in erows if int(r[4]) <= 0] == [(r[0], r[1]) for r in rrows]
    dev = {(r[0], r[1], r[4]): r for r in (l.rstrip("\n").split("\t") for l in open(p("dev_expl")))}
    hit = 0
    for r in erows:                                                  # the same pair explained on either path: the same call
        d = dev.get((r[0], r[1], r[4]))
        if d is not None:
            hit += 1
            assert d[3:] == r[3:] and abs(float(d[2]) - float(r[2])) <= 1e-5
    assert hit >= len(erows) // 2


def _write_dataset(tmp_path, U=60, I=80, H=3, W=3, C=64, seed=3):
    train, val, test = synth.make_interactions(U, I, per_user=8, seed=seed)
    root = str(tmp_path / "data")
    synth.write_dataset(root, "toy", train, val, test, I)
    d = os.path.join(root, "toy", "original", "features", "cnn_vgg19_fc2")
    os.makedirs(d, exist_ok=True)
    rs = np.random.RandomState(seed)
    maps = np.abs(rs.standard_normal((I, 1, H, W, C))).astype(np.float32)
    for i in range(I):
        np.save(os.path.join(d, "%d.npy" % i), maps[i])
    return root, train, val, maps.reshape(I, H * W, C)


def test_cli_writes_explanations_next_to_unchanged_recommendations(tmp_path):
    from fashionvisualexpl_recommend_amd import train_rec
    root, train, val, maps = _write_dataset(tmp_path)
    # --batch_size 1: a step then adds at most one term to a gradient row, so that two runs of the same seed agree bit for bit
    # (larger batches sum a row's terms with float atomics in arrival order) and the files can be compared byte by byte
    common = ["--rec", "acf", "--dataset", "toy", "--data_root", root, "--epochs", "2", "--batch_size", "1", "--embed_k", "16",
              "--layers_component", "32", "1", "--layers_item", "16", "1", "--reg", "0.01", "--top_k", "5"]
    res = [str(tmp_path / "res0"), str(tmp_path / "res1")]
    train_rec.train(common + ["--results_root", res[0]])
    train_rec.train(common + ["--results_root", res[1], "--acf_explain", "3"])
    m = train_rec._last_model
    rdir = [os.path.join(r, "rec_results", "toy", "acf") for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] if "expl-" in f]
    dp = m.directory_parameters
    assert dp.endswith("-comp_[32, 1]-item_[16, 1]")
    assert [f for f in files[1] if "expl-" not in f] == files[0]
    pairs = [(f, f.replace("recs-", "expl-", 1)) for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(pairs) == 2 and all(x in files[1] for _, x in pairs)
    assert "expl-2-%s.tsv" % dp in files[1] and any(f.startswith("best-expl-") for f in files[1])
    ev = m.eval_lists()
    for recs, expl in pairs:
        assert open(os.path.join(rdir[0], recs), "rb").read() == open(os.path.join(rdir[1], recs), "rb").read()
        rrows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], recs))]
        erows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], expl))]
        assert all(len(r) == 10 for r in erows)
        firsts = [r for r in erows if int(r[4]) <= 0]                 # the first row of every (u, i)
        assert [(r[0], r[1]) for r in firsts] == [(r[0], r[1]) for r in rrows]
        for a, b in zip(firsts, rrows):
            assert abs(float(a[2]) - float(b[2])) <= 1e-5
        at = 0
        for u, i, _ in rrows:                                        # ranks 0, 1, 2 per pair, then the next pair
            L = min(3, len(ev[int(u)]))
            blk = erows[at:at + L]
            assert [(r[0], r[1], int(r[4])) for r in blk] == [(u, i, s) for s in range(L)]
            assert all(int(r[5]) in ev[int(u)] and 0 <= int(r[8]) < 9 for r in blk)
            c = [float(r[7]) for r in blk]
            assert c == sorted(c, reverse=True)
            at += L
        assert at == len(erows)
