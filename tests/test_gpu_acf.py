"""ACF on the MI355X against the float64 restatement of ACF.py (tests/acf_ref.py): user profiles g'_u over feature-map shapes,
widths and history lengths (0 .. 3 000, duplicated and shared items), fp32 and bf16 features, score_pairs, predict_all, one sgd
step with reg > 0, 20 adam_tf23 steps in both Adam forms, the detached reg = 0 step, snapshots, range errors and the CLI."""
import os

import numpy as np
import pytest
import torch

from acf_ref import ACFRef, random_tables
from fashionvisualexpl_recommend_amd import _ffi, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _features(rs, I, M, C, dtype):
    F = (np.abs(rs.standard_normal((I, M, C))) * (rs.random_sample((I, M, C)) < 0.5)).astype(np.float32)
    return orc.bf16_round(F) if dtype == "bf16" else F


def _lists(rs, U, I, lens):
    return [sorted(rs.choice(I, n, replace=n > I).tolist()) if n else [] for n in lens]


def _engine(t, F, lists, dtype="fp32", optimizer="sgd", lr=0.05, reg=0.0, B=256, eval_lists=None):
    from fashionvisualexpl_recommend_amd.engine import Engine
    U, k = t["Gu"].shape
    I = t["Gi"].shape[0]
    e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=k, feat_dtype=dtype, optimizer=optimizer, lr=lr, reg=reg,
               max_batch=B)
    return e.bind_acf(t["Gu"], t["Gi"], t["Bi"], F, t["Pi"], {n: t[n] for n in _ffi.ACF_WEIGHTS}, lists, eval_lists)


SHAPES = [  # M, C, k, h, a
    (1, 200, 16, 64, 64), (9, 512, 128, 64, 64), (49, 512, 16, 32, 48), (49, 2048, 128, 64, 64), (196, 200, 16, 64, 64),
]


@pytest.mark.parametrize("M,C,k,h,a,dtype", [s + ("fp32",) for s in SHAPES] + [s + ("bf16",) for s in SHAPES if s[1] % 8 == 0])
def test_profiles_against_fp64(M, C, k, h, a, dtype):
    rs = np.random.RandomState(M + C + k)
    U, I = 12, 40
    t = random_tables(rs, U, I, k, C, h, a, scale=10.0)
    F = _features(rs, I, M, C, dtype)
    lens = [0, 1, 2, 3000, 5, 40, 7, 1, 0, 3, 17, 2]
    lists = _lists(rs, U, I, lens)
    lists[4] = [3, 3, 3, 9, 9]                                       # duplicated history items
    e = _engine(t, F, lists, dtype)
    ref = ACFRef(t, F)
    users = list(range(U)) + [3, 5, 5]                               # duplicated users
    got = e.acf_profiles(users).cpu().double()
    want = ref.profiles(users, lists)
    err = (got - want).abs().max().item()
    # operands: |Gu| <= 0.6, |Pi| ~ 0.1; fp32 rounding of g_u plus a softmax-weighted mean of Pi rows
    assert err <= 1e-5, err
    e.sync_check()


def test_profiles_other_histories_and_score_pairs():
    rs = np.random.RandomState(5)
    U, I, M, C, k = 20, 50, 9, 64, 16
    t = random_tables(rs, U, I, k, C, 64, 64, scale=10.0)
    F = _features(rs, I, M, C, "fp32")
    train = _lists(rs, U, I, rs.randint(0, 12, U))
    other = _lists(rs, U, I, rs.randint(0, 30, U))
    e = _engine(t, F, train)
    ref = ACFRef(t, F)
    got = e.acf_profiles(range(U), other).cpu().double()
    assert (got - ref.profiles(range(U), other)).abs().max().item() <= 1e-5
    u = rs.randint(0, U, 100)
    i = rs.randint(0, I, 100)
    x = e.score_pairs(u, i).cpu().double()
    assert (x - ref.call(u, i, train)).abs().max().item() <= 1e-5
    # predict_all: evaluation histories (train + validation)
    val = [[int(rs.randint(I))] for _ in range(U)]
    ev = [a + b for a, b in zip(train, val)]
    e2 = _engine(t, F, train, eval_lists=ev)
    got = e2.score_block(0, U).cpu().double()
    assert (got - ref.predict_all(ev)).abs().max().item() <= 1e-5


def _batch(rs, U, I, B):
    return rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, I, B)


def _compare_tables(e, ref, atol, tag=""):
    for n in ("Gu", "Gi", "Pi") + tuple(_ffi.ACF_WEIGHTS):
        got = e.t[n].cpu().double().reshape(ref.p[n].shape)
        err = (got - ref.p[n]).abs().max().item()
        assert err <= atol, (tag, n, err)


def test_sgd_step_reg_positive():
    rs = np.random.RandomState(11)
    U, I, M, C, k = 30, 60, 9, 128, 16
    t = random_tables(rs, U, I, k, C, 64, 64, scale=10.0)
    F = _features(rs, I, M, C, "fp32")
    lists = _lists(rs, U, I, rs.randint(0, 15, U))
    e = _engine(t, F, lists, reg=0.1, lr=0.05)
    ref = ACFRef(t, F, reg=0.1)
    batch = _batch(rs, U, I, 200)
    want = ref.step(batch, lists, "sgd", 0.05)
    got = float(e.step(*(torch.as_tensor(b, dtype=torch.int32, device=e.device) for b in batch)).item())
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    _compare_tables(e, ref, 1e-6)
    e.sync_check()


@pytest.mark.parametrize("lazy", ["0", "1"])
def test_adam_20_steps(lazy, monkeypatch):
    monkeypatch.setenv("BPRX_ADAM_LAZY", lazy)
    rs = np.random.RandomState(13)
    U, I, M, C, k = 30, 60, 9, 128, 16
    t = random_tables(rs, U, I, k, C, 32, 48, scale=10.0)
    F = _features(rs, I, M, C, "fp32")
    lists = _lists(rs, U, I, rs.randint(0, 15, U))
    e = _engine(t, F, lists, optimizer="adam_tf23", reg=0.05, lr=1e-3, B=64)
    assert not e.adam_is_lazy()                                   # an ACF handle always sweeps
    ref = ACFRef(t, F, reg=0.05)
    for s in range(20):
        batch = _batch(rs, U, I, 64)
        want = ref.step(batch, lists, "adam_tf23", 1e-3)
        got = float(e.step(*(torch.as_tensor(b, dtype=torch.int32, device=e.device) for b in batch)).item())
        assert abs(got - want) <= 1e-4 * abs(want), (s, got, want)
    _compare_tables(e, ref, 2e-5, "adam")


def test_reg_zero_leaves_all_but_gi_bit_unchanged():
    rs = np.random.RandomState(17)
    U, I, M, C, k = 30, 60, 9, 64, 16
    t = random_tables(rs, U, I, k, C, 64, 64)
    F = _features(rs, I, M, C, "fp32")
    lists = _lists(rs, U, I, rs.randint(0, 15, U))
    for opt in ("sgd", "adam_tf23"):
        e = _engine(t, F, lists, optimizer=opt, reg=0.0, lr=0.01)
        before = {n: v.clone() for n, v in e.t.items()}
        for _ in range(5):
            e.step(*(torch.as_tensor(b, dtype=torch.int32, device=e.device) for b in _batch(rs, U, I, 128)))
        for n in ("Gu", "Pi") + tuple(_ffi.ACF_WEIGHTS):
            assert torch.equal(e.t[n], before[n]), (opt, n)
        assert not torch.equal(e.t["Gi"], before["Gi"])


def test_range_error_and_handle_stays_usable():
    rs = np.random.RandomState(19)
    U, I, M, C, k = 10, 20, 4, 64, 16
    t = random_tables(rs, U, I, k, C, 64, 64)
    F = _features(rs, I, M, C, "fp32")
    lists = _lists(rs, U, I, rs.randint(1, 6, U))
    e = _engine(t, F, lists)
    bad = [list(l) for l in lists]
    bad[2] = [1, 10 ** 6]
    e.acf_profiles([2], bad)
    with pytest.raises(_ffi.BprxError) as ex:
        e.sync_check()
    assert ex.value.code == _ffi.E_RANGE
    ref = ACFRef(t, F)
    assert (e.acf_profiles(range(U)).cpu().double() - ref.profiles(range(U), lists)).abs().max().item() <= 1e-5
    e.sync_check()


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


def test_snapshot_restore_continues_the_run(tmp_path):
    from argparse import Namespace
    from fashionvisualexpl_recommend_amd import models
    rs = np.random.RandomState(23)
    U, I = 40, 50
    train, val, test = synth.make_interactions(U, I, per_user=8, seed=7)
    data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=val, test_list=test,
                     params=Namespace(batch_eval=128))
    params = Namespace(epochs=1, batch_size=32, embed_k=16, lr=1e-3, reg=0.05, top_k=5, dataset="toy", rec="acf",
                       layers_component=[32, 1], layers_item=[32, 1], optimizer="adam_tf23", dtype="fp32")
    F = np.abs(rs.standard_normal((I, 4, 64))).astype(np.float32)
    m = models.ACF(data, params, features=F)
    batches = [_batch(rs, U, I, 32) for _ in range(6)]
    for b in batches[:3]:
        m.train_step(b)
    sd = m.state_dict()
    for b in batches[3:]:
        m.train_step(b)
    want = {n: v.clone() for n, v in m.engine.t.items()}
    m.load_state_dict(sd)
    for b in batches[3:]:
        m.train_step(b)
    for n, v in want.items():                                    # (duplicate rows are summed with float atomics)
        assert torch.allclose(m.engine.t[n], v, rtol=0, atol=1e-6), n


def test_cli_end_to_end(tmp_path):
    import pickle
    from fashionvisualexpl_recommend_amd import train_rec
    root, train, val, maps = _write_dataset(tmp_path)
    res = str(tmp_path / "res")
    out = train_rec.train(["--rec", "acf", "--dataset", "toy", "--data_root", root, "--results_root", res, "--epochs", "2",
                           "--batch_size", "64", "--embed_k", "16", "--layers_component", "32", "1", "--layers_item", "16", "1",
                           "--reg", "0.01", "--top_k", "5"])
    m = train_rec._last_model
    rdir = os.path.join(res, "rec_results", "toy", "acf")
    files = os.listdir(rdir)
    dp = m.directory_parameters
    assert dp.endswith("-comp_[32, 1]-item_[16, 1]")
    assert "results-metrics-%s.pkl" % dp in files
    assert any(f.startswith("recs-2-") for f in files) and any(f.startswith("best-recs-") for f in files)
    with open(os.path.join(rdir, "results-metrics-%s.pkl" % dp), "rb") as f:
        r = pickle.load(f)
    assert set(r) == {1, 2} and 0.0 <= r[1]["hr_v"] <= 1.0
    # the trained model's predict_all equals the fp64 restatement on the same tables
    ref = ACFRef({n: v.cpu().numpy() for n, v in m.engine.t.items() if n in ("Gu", "Gi", "Pi") + tuple(_ffi.ACF_WEIGHTS)}, maps)
    got = m.predict_all().tensor.cpu().double()
    assert (got - ref.predict_all(m.eval_lists())).abs().max().item() <= 1e-5
    assert out
