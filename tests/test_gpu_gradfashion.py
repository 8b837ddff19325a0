"""GradFashion on the MI355X against the float64 autograd restatement (tests/gradfashion_ref.py): scoring, one sgd step
(all eight tables and the loss), 20 Adam steps in both Adam forms and in every step mode, the explanations, snapshot
restore, and the CLI end to end.  Feature widths Dc = 100, De = 290: D = 390 is padded (to 400 for fp32, 512 for bf16)."""
from argparse import Namespace

import os

import numpy as np
import pandas as pd
import pytest
import torch

import torch_ref
from fashionvisualexpl_recommend_amd import configs, synth
from gradfashion_ref import GradFashionRef
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

Dc, De = 100, 290
PAD = {"fp32": 400, "bf16": 512}


def _setup(dtype, U=300, I=600, k=16, d=12, ec=8, ee=12, seed=0, bi_scale=1.0):
    rs = np.random.RandomState(seed)
    Fc, Fe = synth.make_features(I, Dc, seed=seed), synth.make_features(I, De, seed=seed + 7)
    Fc, Fe = (Fc / np.abs(Fc).max()).astype(np.float32), (Fe / np.abs(Fe).max()).astype(np.float32)
    if dtype == "bf16":
        Fc, Fe = orc.bf16_round(Fc), orc.bf16_round(Fe)
    t = dict(Gu=synth.glorot_uniform(rs, U, k), Gi=synth.glorot_uniform(rs, I, k),
             Bi=(rs.uniform(-1, 1, I) * bi_scale).astype(np.float32), Tu=synth.glorot_uniform(rs, U, d),
             Ec=synth.glorot_uniform(rs, Dc, ec), Ee=synth.glorot_uniform(rs, De, ee), E=synth.glorot_uniform(rs, ec + ee, d),
             Bp=synth.glorot_uniform(rs, ec + ee, 1).reshape(-1), Fc=Fc, Fe=Fe)
    F = np.zeros((I, PAD[dtype]), np.float32)
    F[:, :Dc], F[:, Dc:Dc + De] = Fc, Fe
    return t, F


def _engine(t, F, dtype, optimizer="sgd", lr=0.05, reg=0.1, B=256, **kw):
    from fashionvisualexpl_recommend_amd.engine import Engine
    U, k = t["Gu"].shape
    I, d = t["Gi"].shape[0], t["Tu"].shape[1]
    e = Engine(model="vbpr", num_users=U, num_items=I, embed_k=k, embed_d=d, feat_dim=F.shape[1], feat_dtype=dtype,
               optimizer=optimizer, lr=lr, reg=reg, max_batch=B, **kw)
    return e.bind_factored(t["Gu"], t["Gi"], t["Bi"], t["Tu"], F, t["Ec"], t["Ee"], t["E"], t["Bp"], Dc, De, neg_bias_reg=1.0)


def _score_bound(ref, u, i, dtype):
    """|got - want| bound: a rounding unit of the operands times the sum of the absolute terms of each score."""
    p = ref.p
    u, i = torch.as_tensor(u).long(), torch.as_tensor(i).long()
    E, Bp = ref.effective()
    Fi = torch.cat([ref.Fc[i], ref.Fe[i]], 1).abs()
    vis = ((p["Tu"][u].abs() @ E.abs().T) * Fi).sum(1) + Fi @ Bp.abs()
    scale = p["Bi"][i].abs() + (p["Gu"][u] * p["Gi"][i]).abs().sum(1) + vis
    return (1e-5 if dtype == "fp32" else 2.0 ** -8) * scale.numpy() + 1e-6


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_scores_against_fp64(dtype):
    t, F = _setup(dtype)
    e = _engine(t, F, dtype)
    ref = GradFashionRef(t, reg=0.1)
    rs = np.random.RandomState(1)
    u, i = rs.randint(300, size=256), rs.randint(600, size=256)
    got = e.score_pairs(u, i).cpu().numpy()
    want = ref.call(u, i)[0].numpy()
    assert (np.abs(got - want) <= _score_bound(ref, u, i, dtype)).all(), np.abs(got - want).max()
    E, Bp = ref.effective()                                     # the composed projection the handle scores with
    np.testing.assert_allclose(e.t["E_eff"][:Dc + De].cpu().numpy(), E.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(e.t["Bp_eff"][:Dc + De].cpu().numpy(), Bp.numpy(), rtol=1e-5, atol=1e-6)
    assert not e.t["E_eff"][Dc + De:].any() and not e.t["Bp_eff"][Dc + De:].any()
    blk = e.score_block(0, 300).cpu().numpy()
    allw = ref.predict_all().numpy()
    uu, ii = np.meshgrid(np.arange(300), np.arange(600), indexing="ij")
    bound = _score_bound(ref, uu.reshape(-1), ii.reshape(-1), dtype).reshape(300, 600)
    assert (np.abs(blk - allw) <= bound).all(), np.abs(blk - allw).max()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_sgd_step_all_tables_and_loss(dtype):
    """reg 0.1 and Bi ~ U(-1, 1): the negative-bias factor (1 here, 0.1 in VBPR) moves the loss by ~0.9 reg sum(Bi_j^2) ~ 8 and
    every negative's bias by ~0.009 -- far outside the tolerances."""
    lr, reg = 0.05, 0.1
    t, F = _setup(dtype)
    e = _engine(t, F, dtype, lr=lr, reg=reg)
    ref = GradFashionRef(t, reg=reg)
    rs = np.random.RandomState(2)
    u, i, j = (torch.as_tensor(rs.randint(n, size=256).astype(np.int32), device="cuda") for n in (300, 600, 600))
    loss = float(e.step(u, i, j).item())
    e.sync_check()
    want_loss, g = ref.train_step(u.cpu(), i.cpu(), j.cpu(), "sgd", lr)
    assert loss == pytest.approx(want_loss, rel=1e-5 if dtype == "fp32" else 1e-3)
    tol = 1e-4 if dtype == "fp32" else 2e-2
    for n in ("Gu", "Gi", "Bi", "Tu", "Ec", "Ee", "E", "Bp"):
        got = e.t[n].cpu().double().reshape(-1)
        want = ref.p[n].reshape(-1)
        err = (got - want).abs().max().item()
        assert err <= tol * lr * g[n].abs().max().item() + 1e-7, (n, err, g[n].abs().max().item())
    E, Bp = GradFashionRef(dict(t, **{n: e.t[n] for n in ("Ec", "Ee", "E", "Bp")}), reg).effective()
    np.testing.assert_allclose(e.t["E_eff"][:Dc + De].cpu().numpy(), E.numpy(), rtol=1e-5, atol=1e-6)   # recomposed from
    np.testing.assert_allclose(e.t["Bp_eff"][:Dc + De].cpu().numpy(), Bp.numpy(), rtol=1e-5, atol=1e-6)  # the moved factors


def _adam_run(monkeypatch, env, I, form, steps=20, dtype="fp32"):
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    monkeypatch.setenv("BPRX_ADAM_LAZY", "1" if form == "lazy" else "0")
    lr, reg, B = 2e-3, 1e-3, 256
    t, F = _setup(dtype, U=400, I=I, bi_scale=0.01)
    e = _engine(t, F, dtype, optimizer="adam_tf23", lr=lr, reg=reg, B=B)
    assert e.adam_is_lazy() == (form == "lazy")
    ref = GradFashionRef(t, reg=reg)
    rs = np.random.RandomState(3)
    noise = {n: 3e-5 for n in ("Gu", "Gi", "Bi", "Tu", "Ec", "Ee", "E", "Bp")}
    for step in range(1, steps + 1):
        ref.load(e.t, step - 1)
        u, i, j = (torch.as_tensor(rs.randint(n, size=B).astype(np.int32), device="cuda") for n in (400, I, I))
        loss = float(e.step(u, i, j).item())
        e.sync_check()
        want_loss, g = ref.train_step(u.cpu(), i.cpu(), j.cpu(), "adam_tf23", lr)
        assert loss == pytest.approx(want_loss, rel=1e-5), step
        got = {n: v.cpu().double() for n, v in e.t.items() if n not in ("F", "E_eff", "Bp_eff")}
        want = ref.state()
        grads = {n: g[n].reshape(want[n].shape) for n in g}
        absg = {n: torch.full_like(want[n], float(grads[n].abs().max()) + 1e-30) for n in g}     # table-wide gradient scale
        torch_ref.assert_adam_close(got, want, grads, absg, lr, noise, 1e-3, tag="step %d" % step)
    return e


@pytest.mark.parametrize("form", ["lazy", "sweep"])
def test_twenty_adam_steps(monkeypatch, form):
    _adam_run(monkeypatch, {}, 600, form)


@pytest.mark.parametrize("env,I", [({"BPRX_LIST_MODE": "0"}, 5000), ({"BPRX_LIST_MODE": "2"}, 5000),
                                   ({"BPRX_ITEM_MODE": "0"}, 400), ({"BPRX_ITEM_MODE": "2"}, 400)])
def test_twenty_adam_steps_every_step_mode(monkeypatch, env, I):
    """List mode (batch 256 over 5 000 items: its housekeeping -- W rows, multiplicities, the other cursor -- runs in the
    factored step's end) and both item modes, incl. occurrence segments at 2B >= I."""
    _adam_run(monkeypatch, env, I, "lazy")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_explain_pairs_against_gradient_times_input(dtype):
    t, F = _setup(dtype)
    e = _engine(t, F, dtype)
    rs = np.random.RandomState(4)
    u, i = (torch.as_tensor(rs.randint(300, size=64).astype(np.int32), device="cuda"),
            torch.as_tensor(rs.randint(600, size=64).astype(np.int32), device="cuda"))
    for _ in range(3):                                          # away from the initial tables
        e.step(u, i, torch.as_tensor(rs.randint(600, size=64).astype(np.int32), device="cuda"))
    ref = GradFashionRef(t, reg=0.1).load(e.t, 0)
    pu, pi = rs.randint(300, size=2000), rs.randint(600, size=2000)
    got = e.explain_pairs(pu, pi).cpu().numpy()
    want = np.concatenate([ref.predict_ui_grads(int(a), int(b)) for a, b in zip(pu[:50], pi[:50])])
    np.testing.assert_allclose(ref.explain_closed_form(pu[:50], pi[:50]), want, rtol=0, atol=1e-12)
    want = ref.explain_closed_form(pu, pi)
    scale = ref.explain_scale(pu, pi)
    assert (np.abs(got - want) <= 1e-5 * (np.abs(want) + scale)).all(), np.abs(got - want).max()
    e.sync_check()


def _data(U, I, params, seed=5):
    tr, va, te = synth.make_interactions(U, I, per_user=12, seed=seed)
    return Namespace(num_users=U, num_items=I, training_list=tr, validation_list=va, test_list=te, params=params)


def _params(**kw):
    p = dict(dataset="gf", validation=True, batch_size=128, epochs=1, batch_eval=128, embed_k=16, embed_d=12, embed_color=8,
             embed_edges=12, lr=2e-3, reg=1e-3, top_k=10, verbose=-1, restore_epochs=1, rec="grad_fashion", best_metric="ndcg",
             optimizer="adam_tf23", init_seed=5, dtype="fp32")
    p.update(kw)
    return Namespace(**p)


@pytest.mark.parametrize("opt", ["adam_tf23", "sgd"])
def test_state_dict_restore_then_step(opt):
    """load_state_dict (factor tables + slots + step counter; E_eff recomposed) followed by steps = the uninterrupted run."""
    from fashionvisualexpl_recommend_amd.models import GradFashion
    U, I = 200, 300
    t, _ = _setup("fp32", U=U, I=I)
    p = _params(optimizer=opt)
    m = GradFashion(_data(U, I, p), p, features=(t["Fc"], t["Fe"]))
    rs = np.random.RandomState(6)
    batches = [tuple(torch.as_tensor(rs.randint(n, size=128).astype(np.int32), device="cuda") for n in (U, I, I)) for _ in range(5)]
    for b in batches[:2]:
        m.engine.step(*b)
    snap = m.state_dict()
    for b in batches[2:]:
        m.engine.step(*b)
    want = {n: v.clone() for n, v in m.engine.t.items()}
    for b in batches[:1]:                                       # wander off, then restore
        m.engine.step(*b)
    m.load_state_dict(snap)
    for b in batches[2:]:
        m.engine.step(*b)
    for n, v in want.items():                                   # (row gradients meet in fp32 atomics: order-level noise only)
        torch.testing.assert_close(m.engine.t[n], v, rtol=1e-5, atol=1e-6, msg=n)


def test_cli_end_to_end_against_fp64(tmp_path, capsys, opt="adam_tf23", lr=1e-2):
    """train_rec --rec grad_fashion, 1 000 x 2 000, 3 epochs on the reference index stream: HR@10 / NDCG@10 against the fp64
    restatement trained on the same stream, and the explanation rows written to the recs-* path."""
    from fashionvisualexpl_recommend_amd import train_rec
    U, I, bs, epochs, reg = 1000, 2000, 256, 3, 1e-3
    tr, va, te = synth.make_interactions_clustered(U, I, per_user=22, clusters=20, p_in=0.9, seed=2024)
    synth.write_dataset(str(tmp_path), "gfc", tr, va, te, I)
    rs = np.random.RandomState(9)
    color, edges = rs.rand(I, Dc).astype(np.float32) * 3, synth.make_features(I, De, seed=11)
    synth.write_grad_fashion_features(str(tmp_path), "gfc", color, edges)
    train_rec.train(["--rec", "grad_fashion", "--dataset", "gfc", "--data_root", str(tmp_path), "--results_root",
                     str(tmp_path / "results"), "--epochs", str(epochs), "--batch_size", str(bs), "--embed_k", "32",
                     "--embed_d", "12", "--embed_color", "8", "--embed_edges", "16", "--lr", str(lr), "--top_k", "10",
                     "--list_of_regs", str(reg), "--optimizer", opt, "--init_seed", "3"])
    model = train_rec._last_model
    got = model.results[epochs]
    # the restatement, from the model's own initial tables (same seed) on the same index stream
    g = np.random.RandomState(3)
    init = dict(Bi=np.zeros(I, np.float32), Gu=synth.glorot_uniform(g, U, 32), Gi=synth.glorot_uniform(g, I, 32),
                Bp=synth.glorot_uniform(g, 24, 1), E=synth.glorot_uniform(g, 24, 12), Tu=synth.glorot_uniform(g, U, 12),
                Ec=synth.glorot_uniform(g, Dc, 8), Ee=synth.glorot_uniform(g, De, 16),
                Fc=color / np.abs(color).max(), Fe=edges / np.abs(edges).max())
    ref = GradFashionRef(init, reg=reg)
    u, i, j = orc.sample_ref_stream(tr, I, bs, epochs)
    for s in range(0, len(u), bs):
        ref.train_step(u[s:s + bs], i[s:s + bs], j[s:s + bs], opt, lr)
    want = orc.evaluate(ref.predict_all().numpy().astype(np.float32), tr, va, te, 10)
    for key in ("hr_v", "ndcg_v", "hr_t", "ndcg_t"):
        assert abs(got[key] - want[key]) <= 1e-3, (key, got[key], want[key])
    assert want["hr_t"] > 0.02 and got["hr_t"] > 0.02          # > 4x the random-ranking level: the comparison is informative
    path = os.path.join(str(tmp_path / "results"), "rec_results", "gfc", "grad_fashion",
                        "recs-%d-%s.tsv" % (epochs, model.directory_parameters))
    df = pd.read_csv(path, sep="\t", names=["USER_ID", "ITEM_ID", "COLOR", "EDGES"])       # get_explanations.py:19-21
    users = np.concatenate([[uu] * (len(tr[uu]) + len(va[uu]) + len(te[uu])) for uu in range(U)])
    items = np.concatenate([tr[uu] + va[uu] + te[uu] for uu in range(U)])
    np.testing.assert_array_equal(df["USER_ID"].values, users)
    np.testing.assert_array_equal(df["ITEM_ID"].values, items)
    gx = df[["COLOR", "EDGES"]].values
    # the written rows are the attribution of the trained tables: against the restatement evaluated at the engine's tables ...
    own = GradFashionRef(dict(init), reg=reg).load(model.engine.t, 0)
    wx, sc = own.explain_closed_form(users, items), own.explain_scale(users, items)
    assert (np.abs(gx - wx) <= 1e-4 * np.abs(wx) + 1e-5 * sc).all(), np.abs(gx - wx).max()
    # ... and against the fp64 run itself: 234 Adam steps in fp32 drift the tables by ~1e-4 of the attribution's term scale
    wx, sc = ref.explain_closed_form(users, items), ref.explain_scale(users, items)
    assert np.median(np.abs(gx - wx) / (np.abs(wx) + sc)) <= 1e-5
    assert (np.abs(gx - wx) <= 1e-3 * (np.abs(wx) + sc)).all(), np.abs(gx - wx).max()
    assert any(f.startswith("best-recs-") for f in os.listdir(os.path.dirname(path)))


def test_cli_bf16_philox_runs(tmp_path):
    from fashionvisualexpl_recommend_amd import train_rec
    U, I = 300, 700
    tr, va, te = synth.make_interactions_clustered(U, I, per_user=14, clusters=10, p_in=0.9, seed=3)
    synth.write_dataset(str(tmp_path), "gfb", tr, va, te, I)
    synth.write_grad_fashion_features(str(tmp_path), "gfb", np.random.RandomState(1).rand(I, Dc), synth.make_features(I, De))
    res = train_rec.train(["--rec", "grad_fashion", "--dataset", "gfb", "--data_root", str(tmp_path), "--results_root",
                           str(tmp_path / "results"), "--epochs", "2", "--batch_size", "128", "--embed_k", "16",
                           "--embed_d", "8", "--dtype", "bf16", "--sampler", "philox", "--lr", "0.005"])
    assert sorted(res[0]) == [1, 2] and res[0][2]["hr_t"] > 0
    d = os.path.join(str(tmp_path / "results"), "rec_results", "gfb", "grad_fashion")
    f = [x for x in os.listdir(d) if x.startswith("recs-2-")][0]
    df = pd.read_csv(os.path.join(d, f), sep="\t", names=["USER_ID", "ITEM_ID", "COLOR", "EDGES"])
    assert len(df) == sum(len(a) + len(b) + len(c) for a, b, c in zip(tr, va, te)) and np.isfinite(df[["COLOR", "EDGES"]].values).all()
