"""ACF's full-gradient mode (bprx_acf_set_gradient, BPRX_ACF_GRAD_FULL) on the MI355X against float64 autograd over the
restatement (tests/acf_full_ref.py): one sgd step on empty / duplicated / shared / 3 000-item histories with duplicated users,
fp32 and bf16 features, reg 0 and 0.1; one sgd step over test_gpu_acf.py's shape grid; 20 adam_tf23 steps; what moves at reg 0;
the default step bit for bit; range errors; snapshots; the CLI.

Tolerances: per table, acf_full_ref.TOL_MULT x the max-abs deviation of the SAME restatement run in float32 on the CPU from the
float64 one (reasons for the multiple: acf_full_ref.py).  Every comparison first asserts that the float64 run met no relu input
closer to zero than RELU_DELTA.  The figures of the first GPU run are in DESIGN.md section 9."""
import os

import numpy as np
import pytest
import torch

import acf_full_ref as R
from acf_ref import ACFRef, random_tables
from fashionvisualexpl_recommend_amd import _ffi, synth

pytestmark = pytest.mark.gpu

SGD_LR = 0.5          # a large step: the tables after it carry the gradient at half weight, not at 1/20


def _engine(t, F, lists, dtype="fp32", optimizer="sgd", lr=0.05, reg=0.0, B=256, gradient=None):
    from fashionvisualexpl_recommend_amd.engine import Engine
    U, k = t["Gu"].shape
    I = t["Gi"].shape[0]
    e = Engine(model="bprmf", num_users=U, num_items=I, embed_k=k, feat_dtype=dtype, optimizer=optimizer, lr=lr, reg=reg,
               max_batch=B)
    kw = {} if gradient is None else {"gradient": gradient}
    return e.bind_acf(t["Gu"], t["Gi"], t["Bi"], F, t["Pi"], {n: t[n] for n in _ffi.ACF_WEIGHTS}, lists, None, **kw)


def _dev(e, batch):
    return tuple(torch.as_tensor(np.asarray(b), dtype=torch.int32, device=e.device) for b in batch)


def _compare(e, t64, t32, tag):
    allow = R.allowances(t64, t32)
    bad = []
    for n in R.NAMES:
        got = e.t[n].cpu().double().numpy().reshape(t64[n].shape)
        err = float(np.abs(got - t64[n]).max())
        print("%s %-16s fp32 restatement %.3e  allowance %.3e  gpu %.3e" % (tag, n, allow[n] / R.TOL_MULT, allow[n], err))
        if not err <= allow[n]:
            bad.append((n, err, allow[n]))
    assert not bad, (tag, bad)


def _sgd_step_case(t, F, lists, batch, dtype, reg, tag):
    loss64, t64, mr = R.run_sgd(t, F, lists, batch, reg, SGD_LR, torch.float64)
    assert mr > R.RELU_DELTA, mr
    loss32, t32, _ = R.run_sgd(t, F, lists, batch, reg, SGD_LR, torch.float32)
    e = _engine(t, F, lists, dtype, reg=reg, lr=SGD_LR, gradient="full")
    assert e.acf_gradient() == "full"
    got = float(e.step(*_dev(e, batch)).item())
    lallow = max(R.TOL_MULT * abs(loss32 - loss64), 1e-5 * abs(loss64))      # the detached test's 1e-5 relative, or the unit's multiple
    print("%s loss fp32 restatement %.3e allowance %.3e gpu %.3e" % (tag, abs(loss32 - loss64), lallow, abs(got - loss64)))
    assert abs(got - loss64) <= lallow, (got, loss64)
    _compare(e, t64, t32, tag)
    e.sync_check()
    return e


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("reg", [0.0, 0.1])
def test_sgd_step_special_histories(dtype, reg):
    t, F, lists, batch = R.special_case(dtype)
    _sgd_step_case(t, F, lists, batch, dtype, reg, "special/%s/reg%g" % (dtype, reg))


@pytest.mark.parametrize("M,C,k,h,a,dtype", [s + ("fp32",) for s in R.SHAPES] + [s + ("bf16",) for s in R.SHAPES if s[1] % 8 == 0])
def test_sgd_step_shape_grid(M, C, k, h, a, dtype):
    t, F, lists, batch = R.grid_case((M, C, k, h, a), dtype)
    _sgd_step_case(t, F, lists, batch, dtype, 0.1, "grid/M%d/C%d/k%d/%s" % (M, C, k, dtype))


@pytest.mark.parametrize("reg", [0.0, 0.05])
def test_adam_20_steps(reg):
    t, F, lists, batches = R.adam_case(reg)
    l64, t64, mr = R.run_adam(t, F, lists, batches, reg, R.ADAM_LR, torch.float64)
    assert mr > R.RELU_DELTA, mr
    l32, t32, _ = R.run_adam(t, F, lists, batches, reg, R.ADAM_LR, torch.float32)
    e = _engine(t, F, lists, optimizer="adam_tf23", reg=reg, lr=R.ADAM_LR, B=R.ADAM_B, gradient="full")
    for s, b in enumerate(batches):
        got = float(e.step(*_dev(e, b)).item())
        lallow = max(R.TOL_MULT * abs(l32[s] - l64[s]), 1e-4 * abs(l64[s]))  # 1e-4 relative: the detached Adam test's bound
        assert abs(got - l64[s]) <= lallow, (s, got, l64[s])
    _compare(e, t64, t32, "adam/reg%g" % reg)
    e.sync_check()


def test_reg_zero_trains_everything_but_the_two_b1():
    t, F, lists, batch = R.special_case("fp32")
    for opt in ("sgd", "adam_tf23"):
        e = _engine(t, F, lists, optimizer=opt, reg=0.0, lr=0.01, gradient="full")
        before = {n: v.clone() for n, v in e.t.items()}
        for _ in range(3):
            e.step(*_dev(e, batch))
        for n in R.NAMES:
            if n in R.B1_NAMES:
                assert torch.equal(e.t[n], before[n]), (opt, n)       # exactly 2 reg b_1 = 0
            else:
                assert not torch.equal(e.t[n], before[n]), (opt, n)
        e.sync_check()


@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
@pytest.mark.parametrize("reg", [0.0, 0.05])
def test_default_step_did_not_move(opt, reg):
    rs = np.random.RandomState(31)
    U, I, M, C, k, B = 40, 90, 9, 128, 16, 32
    t = random_tables(rs, U, I, k, C, 64, 64, scale=10.0)
    F = R.features(rs, I, M, C, "fp32")
    lists = R.lists_of(rs, I, rs.randint(0, 12, U))
    batches = []
    for _ in range(5):                                               # users, pos and neg items all distinct: no two atomic adds meet
        it = rs.permutation(I)[:2 * B]
        batches.append((rs.permutation(U)[:B], it[:B], it[B:]))
    engines = [_engine(t, F, lists, optimizer=opt, reg=reg, lr=0.01), _engine(t, F, lists, optimizer=opt, reg=reg, lr=0.01, gradient="detached"),
               _engine(t, F, lists, optimizer=opt, reg=reg, lr=0.01)]
    engines[2].acf_set_gradient("full")
    engines[2].acf_set_gradient("detached")
    assert [e.acf_gradient() for e in engines] == ["detached"] * 3
    losses = []
    for e in engines:
        losses.append([float(e.step(*_dev(e, b)).item()) for b in batches])
        e.sync_check()
    assert losses[0] == losses[1] == losses[2]
    for n in engines[0].t:
        assert torch.equal(engines[0].t[n], engines[1].t[n]) and torch.equal(engines[0].t[n], engines[2].t[n]), n
    # and it is the reference's detached step (test_gpu_acf.py's tolerances)
    ref = ACFRef(t, F, reg=reg)
    for b in batches:
        ref.step(b, lists, opt, 0.01)
    for n in R.NAMES:
        err = (engines[2].t[n].cpu().double().reshape(ref.p[n].shape) - ref.p[n]).abs().max().item()
        assert err <= (1e-6 if opt == "sgd" else 2e-5), (n, err)


def test_set_gradient_states():
    from fashionvisualexpl_recommend_amd.engine import Engine
    rs = np.random.RandomState(3)
    e = Engine(model="bprmf", num_users=8, num_items=9, embed_k=16, optimizer="sgd", lr=0.1, reg=0.0, max_batch=16)
    e.bind(Gu=synth.glorot_uniform(rs, 8, 16), Gi=synth.glorot_uniform(rs, 9, 16), Bi=np.zeros(9, np.float32))
    with pytest.raises(_ffi.BprxError) as ex:
        e.acf_set_gradient("full")
    assert ex.value.code == _ffi.E_STATE
    assert e.lib.bprx_acf_get_gradient(e.h) == _ffi.E_STATE
    t, F, lists, _ = R.grid_case(R.SHAPES[0], "fp32")
    e2 = _engine(t, F, lists)
    assert e2.lib.bprx_acf_set_gradient(e2.h, 2) == _ffi.E_INVALID
    assert e2.acf_gradient() == "detached"


def test_range_errors_and_handle_stays_usable():
    t, F, lists, batch = R.grid_case(R.SHAPES[1], "fp32")
    U, I = t["Gu"].shape[0], t["Gi"].shape[0]
    e = _engine(t, F, lists, reg=0.0, lr=0.01, gradient="full")
    for pos_in_batch, col, value in ((0, 0, U + 5), (1, 1, -3), (2, 2, 10 ** 6)):
        bad = [np.array(b).copy() for b in batch]
        bad[col][pos_in_batch] = value
        e.step(*_dev(e, bad))
        with pytest.raises(_ffi.BprxError) as ex:
            e.sync_check()
        assert ex.value.code == _ffi.E_RANGE
    badl = [list(l) for l in lists]
    badl[2] = [1, 10 ** 6]
    e2 = _engine(t, F, badl, reg=0.0, lr=0.01, gradient="full")     # an out-of-range history index: clamped and reported
    e2.step(*_dev(e2, batch))
    with pytest.raises(_ffi.BprxError) as ex:
        e2.sync_check()
    assert ex.value.code == _ffi.E_RANGE
    # the first handle still computes the right step
    e.bind_acf(t["Gu"], t["Gi"], t["Bi"], F, t["Pi"], {n: t[n] for n in _ffi.ACF_WEIGHTS}, lists, None, gradient="full")
    e.set_hyper(SGD_LR, 0.1)
    _, t64, _ = R.run_sgd(t, F, lists, batch, 0.1, SGD_LR, torch.float64)
    _, t32, _ = R.run_sgd(t, F, lists, batch, 0.1, SGD_LR, torch.float32)
    e.step(*_dev(e, batch))
    _compare(e, t64, t32, "after-range-error")
    e.sync_check()


def test_snapshot_restore_continues_a_full_run():
    from argparse import Namespace
    from fashionvisualexpl_recommend_amd import models
    rs = np.random.RandomState(23)
    U, I = 40, 50
    train, val, test = synth.make_interactions(U, I, per_user=8, seed=7)
    data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=val, test_list=test,
                     params=Namespace(batch_eval=128))
    p = dict(epochs=1, batch_size=32, embed_k=16, lr=1e-3, reg=0.05, top_k=5, dataset="toy", rec="acf",
             layers_component=[32, 1], layers_item=[32, 1], optimizer="adam_tf23", dtype="fp32", acf_gradient="full")
    F = np.abs(rs.standard_normal((I, 4, 64))).astype(np.float32)
    m = models.ACF(data, Namespace(**p), features=F)
    assert m.engine.acf_gradient() == "full" and m.directory_parameters.endswith("-grad_full")
    batches = [(rs.randint(0, U, 32), rs.randint(0, I, 32), rs.randint(0, I, 32)) for _ in range(6)]
    for b in batches[:3]:
        m.train_step(b)
    sd = m.state_dict()
    assert sd["acf_gradient"] == "full"
    for b in batches[3:]:
        m.train_step(b)
    want = {n: v.clone() for n, v in m.engine.t.items()}
    assert not torch.equal(want["item.W_0_ix"], sd["item.W_0_ix"])
    m.load_state_dict(sd)
    for b in batches[3:]:
        m.train_step(b)
    for n, v in want.items():                                    # (float atomics: equal up to the order of additions)
        assert torch.allclose(m.engine.t[n], v, rtol=0, atol=1e-6), n
    p["acf_gradient"] = "detached"
    d = models.ACF(data, Namespace(**p), features=F)
    assert "acf_gradient" not in d.state_dict() and not d.directory_parameters.endswith("-grad_full")
    with pytest.raises(ValueError, match="acf_gradient"):
        d.load_state_dict(sd)
    with pytest.raises(ValueError, match="acf_gradient"):
        m.load_state_dict(d.state_dict())


def test_cli_end_to_end_full(tmp_path):
    import pickle
    from fashionvisualexpl_recommend_amd import train_rec
    U, I, H, W, C = 60, 80, 3, 3, 64
    train, val, test = synth.make_interactions(U, I, per_user=8, seed=3)
    root = str(tmp_path / "data")
    synth.write_dataset(root, "toy", train, val, test, I)
    d = os.path.join(root, "toy", "original", "features", "cnn_vgg19_fc2")
    os.makedirs(d, exist_ok=True)
    maps = np.abs(np.random.RandomState(3).standard_normal((I, 1, H, W, C))).astype(np.float32)
    for i in range(I):
        np.save(os.path.join(d, "%d.npy" % i), maps[i])
    res = str(tmp_path / "res")
    out = train_rec.train(["--rec", "acf", "--acf_gradient", "full", "--dataset", "toy", "--data_root", root, "--results_root", res,
                           "--epochs", "2", "--batch_size", "64", "--embed_k", "16", "--layers_component", "32", "1",
                           "--layers_item", "16", "1", "--reg", "0.01", "--top_k", "5"])
    m = train_rec._last_model
    assert m.engine.acf_gradient() == "full"
    dp = m.directory_parameters
    assert dp.endswith("-comp_[32, 1]-item_[16, 1]-grad_full")
    rdir = os.path.join(res, "rec_results", "toy", "acf")
    files = os.listdir(rdir)
    assert "results-metrics-%s.pkl" % dp in files
    assert any(f.startswith("recs-2-") for f in files) and any(f.startswith("best-recs-") for f in files)
    with open(os.path.join(rdir, "results-metrics-%s.pkl" % dp), "rb") as f:
        r = pickle.load(f)
    assert set(r) == {1, 2} and 0.0 <= r[1]["hr_v"] <= 1.0
    ref = ACFRef({n: v.cpu().numpy() for n, v in m.engine.t.items() if n in R.NAMES}, maps.reshape(I, H * W, C))
    got = m.predict_all().tensor.cpu().double()
    assert (got - ref.predict_all(m.eval_lists())).abs().max().item() <= 1e-5
    assert out
