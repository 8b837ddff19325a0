"""GradFashion's factored kernels (k_fact_compose, k_fact_grad, k_fact_update, k_fact_explain) and its step path on the MI355X
at the shapes of tests/gradfashion_shapes.py -- every branch of their launch arithmetic that the one shape family of
tests/test_gpu_gradfashion.py leaves out -- and bf16 handles beyond their first step, where every projection reads [E|Bp]^T
images rebuilt from the recomposed E_eff.  The checker is the float64 restatement (tests/gradfashion_ref.py); the tolerances are
the project's own (fp32: loss 1e-5, tables 1e-4 lr max|g| + 1e-7; bf16: 1e-3 and 2e-2).  tests/test_gradfashion_shapes_cpu.py
shows on the CPU that the inputs are fair and that a stale image would break the bf16 bounds by more than 10x."""
import numpy as np
import pytest
import torch

import gradfashion_shapes as S
import torch_ref
from gradfashion_ref import PARAMS, GradFashionRef
from test_gpu_gradfashion import _score_bound

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16")
GRID = [pytest.param(n, dt, id="%s-%s" % (n, dt)) for n in S.SHAPES for dt in DTYPES]


def _engine(name, t, F, dtype, optimizer="sgd", lr=S.LR, reg=S.REG, B=S.B):
    from fashionvisualexpl_recommend_amd.engine import Engine
    Dc, De = S.shape_of(name)[:2]
    U, k = t["Gu"].shape
    I, d = t["Gi"].shape[0], t["Tu"].shape[1]
    e = Engine(model="vbpr", num_users=U, num_items=I, embed_k=k, embed_d=d, feat_dim=F.shape[1], feat_dtype=dtype,
               optimizer=optimizer, lr=lr, reg=reg, max_batch=B)
    return e.bind_factored(t["Gu"], t["Gi"], t["Bi"], t["Tu"], F, t["Ec"], t["Ee"], t["E"], t["Bp"], Dc, De, neg_bias_reg=1.0)


def _dev(batch):
    return tuple(torch.as_tensor(x, device="cuda") for x in batch)


def _effective_matches(e, name, t, reg=S.REG):
    """E_eff / Bp_eff = the composition of the handle's own factor tables; rows past Dc + De exactly zero."""
    Dc, De = S.shape_of(name)[:2]
    E, Bp = GradFashionRef(dict(t, **{n: e.t[n] for n in ("Ec", "Ee", "E", "Bp")}), reg).effective()
    np.testing.assert_allclose(e.t["E_eff"][:Dc + De].cpu().numpy(), E.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(e.t["Bp_eff"][:Dc + De].cpu().numpy(), Bp.numpy(), rtol=1e-5, atol=1e-6)
    assert not e.t["E_eff"][Dc + De:].any() and not e.t["Bp_eff"][Dc + De:].any()
    return e.t["E_eff"].shape[0] - (Dc + De)


def _tables_close(e, want, bounds, tag):
    """Every table of the handle within its bound of the restatement's; every figure is printed before any is asserted."""
    bad = []
    for n in PARAMS:
        err = float((e.t[n].cpu().double().reshape(-1) - torch.as_tensor(want[n])).abs().max())
        print("%s %-2s bound %.3e  gpu %.3e" % (tag, n, bounds[n], err))
        if not err <= bounds[n]:
            bad.append((n, err, bounds[n]))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("name,dtype", GRID)
def test_bind_composes_and_scores(name, dtype):
    t, F, _ = S.case(name, dtype)
    e = _engine(name, t, F, dtype)
    ref = GradFashionRef(t, reg=S.REG)
    zero_rows = _effective_matches(e, name, t)
    if name in ("exact", "bench"):
        assert zero_rows == 0
    rs = np.random.RandomState(11)
    u, i = rs.randint(S.U, size=64), rs.randint(S.I, size=64)
    got, want = e.score_pairs(u, i).cpu().numpy(), ref.call(u, i)[0].numpy()
    assert (np.abs(got - want) <= _score_bound(ref, u, i, dtype)).all(), np.abs(got - want).max()
    blk, allw = e.score_block(0, S.U).cpu().numpy(), ref.predict_all().numpy()
    uu, ii = np.meshgrid(np.arange(S.U), np.arange(S.I), indexing="ij")
    bound = _score_bound(ref, uu.reshape(-1), ii.reshape(-1), dtype).reshape(S.U, S.I)
    assert (np.abs(blk - allw) <= bound).all(), np.abs(blk - allw).max()
    e.sync_check()


@pytest.mark.parametrize("name,dtype", GRID)
def test_one_sgd_step_all_tables_and_loss(name, dtype):
    t, F, batches = S.case(name, dtype)
    e = _engine(name, t, F, dtype)
    loss = float(e.step(*_dev(batches[0])).item())
    e.sync_check()
    want_loss, g, ref = S.run_sgd(t, batches[:1])
    print("%s-%s loss bound %.3e  gpu %.3e" % (name, dtype, S.LOSS_REL[dtype] * abs(want_loss[0]), abs(loss - want_loss[0])))
    assert loss == pytest.approx(want_loss[0], rel=S.LOSS_REL[dtype])
    _tables_close(e, S.tables_of(ref), {n: S.table_bound(dtype, S.LR, g[0][n]) for n in PARAMS}, "%s-%s" % (name, dtype))
    _effective_matches(e, name, t)                                      # recomposed from the moved factors


@pytest.mark.parametrize("name,dtype", GRID)
def test_explain_pairs_after_three_steps(name, dtype):
    t, F, batches = S.case(name, dtype)
    e = _engine(name, t, F, dtype)
    for b in batches:                                                   # away from the initial tables
        e.step(*_dev(b))
    ref = GradFashionRef(t, reg=S.REG).load(e.t, 0)
    rs = np.random.RandomState(12)
    pu, pi = rs.randint(S.U, size=200), rs.randint(S.I, size=200)
    got = e.explain_pairs(pu, pi).cpu().numpy()
    want, scale = ref.explain_closed_form(pu, pi), ref.explain_scale(pu, pi)
    assert (np.abs(got - want) <= 1e-5 * (np.abs(want) + scale)).all(), np.abs(got - want).max()
    e.sync_check()


@pytest.mark.parametrize("name", S.ADAM_SHAPES)
def test_three_adam_steps_teacher_forced(name):
    """test_gpu_gradfashion._adam_run's comparison (each step of the restatement starts from the handle's own state) on the large
    shapes; on `upd` the loss holds the 2048 block partials of k_fact_update."""
    lr, reg = 2e-3, 1e-3
    t, F, batches = S.case(name, "fp32", bi_scale=0.01)
    e = _engine(name, t, F, "fp32", optimizer="adam_tf23", lr=lr, reg=reg)
    ref = GradFashionRef(t, reg=reg)
    noise = {n: 3e-5 for n in PARAMS}
    for step, b in enumerate(batches, 1):
        ref.load(e.t, step - 1)
        loss = float(e.step(*_dev(b)).item())
        e.sync_check()
        want_loss, g = ref.train_step(*b, "adam_tf23", lr)
        assert loss == pytest.approx(want_loss, rel=1e-5), step
        got = {n: v.cpu().double() for n, v in e.t.items() if n not in ("F", "E_eff", "Bp_eff")}
        want = ref.state()
        grads = {n: g[n].reshape(want[n].shape) for n in g}
        absg = {n: torch.full_like(want[n], float(grads[n].abs().max()) + 1e-30) for n in g}
        torch_ref.assert_adam_close(got, want, grads, absg, lr, noise, 1e-3, tag="%s step %d" % (name, step))
    _effective_matches(e, name, t, reg)


def test_factored_dense_stage_is_reproducible():
    """No atomics in k_fact_grad / k_fact_update / k_fact_compose: two fresh handles stepped once agree bit for bit in the factor
    tables, at the shape where the update strides."""
    t, F, batches = S.case("upd", "fp32")
    out = []
    for _ in range(2):
        e = _engine("upd", t, F, "fp32")
        e.step(*_dev(batches[0]))
        e.sync_check()
        out.append({n: e.t[n].clone() for n in ("Ec", "Ee", "E", "Bp")})
    for n in out[0]:
        assert torch.equal(out[0][n], out[1][n]), n


@pytest.mark.parametrize("name", ["base", "bench"])
def test_bf16_three_free_running_sgd_steps(name):
    """From the second step on every projection reads the bf16 [E|Bp]^T images that k_dense_update rebuilt from the recomposed
    E_eff.  tests/test_gradfashion_shapes_cpu.py: a step computed from the images of the step before moves g_Tu and the loss by
    more than 10x these bounds."""
    t, F, batches = S.case(name, "bf16")
    e = _engine(name, t, F, "bf16")
    want_loss, g, ref = S.run_sgd(t, batches)
    for step, b in enumerate(batches):
        loss = float(e.step(*_dev(b)).item())
        print("%s step %d loss bound %.3e  gpu %.3e" % (name, step + 1, 1e-3 * abs(want_loss[step]), abs(loss - want_loss[step])))
        assert loss == pytest.approx(want_loss[step], rel=S.LOSS_REL["bf16"]), step + 1
    e.sync_check()
    bounds = {n: S.table_bound("bf16", S.LR, sum(s[n] for s in g)) for n in PARAMS}
    _tables_close(e, S.tables_of(ref), bounds, "%s-bf16 3 steps" % name)
    _effective_matches(e, name, t)


ADAM_MODES = [({}, 600), ({"BPRX_LIST_MODE": "0"}, 5000), ({"BPRX_LIST_MODE": "2"}, 5000), ({"BPRX_ITEM_MODE": "0"}, 400),
              ({"BPRX_ITEM_MODE": "2"}, 400)]


@pytest.mark.parametrize("env,I", ADAM_MODES, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) or "default"
                         if isinstance(v, dict) else "I%d" % v)
@pytest.mark.parametrize("name", ["base", "bench"])
def test_bf16_twenty_adam_steps_teacher_forced(monkeypatch, name, env, I):
    """test_gpu_gradfashion._adam_run's sizes (U = 400, B = 256, k = 16, lr 2e-3, reg 1e-3) with bf16 features in every step mode.
    Per step: the loss, and every table's first-moment slot within the bf16 gradient bound carried through one slot update,
    (1 - b1) 2e-2 max|g| + 1e-7 -- a bound on the gradient itself, which Adam's sign amplification at zero slots does not enter."""
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    lr, reg, U, B, steps = 2e-3, 1e-3, 400, 256, 20
    t, F, batches = S.case(name, "bf16", steps=steps, users=U, items=I, k=16, batch=B, bi_scale=0.01)
    e = _engine(name, t, F, "bf16", optimizer="adam_tf23", lr=lr, reg=reg, B=B)
    ref = GradFashionRef(t, reg=reg)
    worst = {n: 0.0 for n in PARAMS}
    for step, b in enumerate(batches, 1):
        ref.load(e.t, step - 1)
        loss = float(e.step(*_dev(b)).item())
        e.sync_check()
        want_loss, g = ref.train_step(*b, "adam_tf23", lr)
        assert loss == pytest.approx(want_loss, rel=S.LOSS_REL["bf16"]), step
        for n in PARAMS:
            err = float((e.t["m_" + n].cpu().double().reshape(-1) - ref.m[n].reshape(-1)).abs().max())
            bound = (1 - torch_ref.B1) * 2e-2 * float(g[n].abs().max()) + 1e-7
            worst[n] = max(worst[n], err / bound)
            assert err <= bound, (step, n, err, bound)
    print("%s %s largest m-slot error / bound: %s" % (name, env, {n: "%.3f" % v for n, v in worst.items()}))
